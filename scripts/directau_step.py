"""ms per DirectAU training step at yelp2018 shape (synthetic, idgrec_amd.synth), d = 64, B = 2048, one JSON line:
the fused step (LightGCN encoder: row-restricted propagation, idg_align_uniform_f32, one backward propagation with Adam
in its epilogue), the same model through forward() + autograd + Adam, and the fused LightGCN (BPR) step at the same B.
Device-event timing after a warm-up.

    python scripts/directau_step.py [--steps 50] [--warmup 10]
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
import utility.utility_data.data_loader as data_loader  # noqa: E402
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
    args = ap.parse_args()
    from models.DirectAU import DirectAU
    from models.LightGCN import LightGCN

    root = tempfile.mkdtemp(prefix="idg_au_step_")
    S.make_dataset(root, "yelp2018", n_test=1)
    cfg = tools.read_configuration(os.path.join(ROOT, "configure", "DirectAU.txt"), "DirectAU")
    cfg.update(dataset="yelp2018", dataset_path=root + "/", sparsity_test="0", embedding_size="64", batch_size="2048")
    data = data_loader.Data(os.path.join(root, "yelp2018"), cfg)
    B = 2048
    np.random.seed(0)
    s = data.sample_data_to_train_all()
    nb = 16
    tri = torch.from_numpy(s[:nb * B]).cuda()
    batches = [tuple(tri[i * B:(i + 1) * B, c].contiguous() for c in range(3)) for i in range(nb)]
    loss = torch.zeros(3, device="cuda")
    out = {"shape": "yelp2018", "d": 64, "B": B, "steps": args.steps}

    tools.set_seed(2024)
    m = DirectAU(cfg, data, torch.device("cuda")).to("cuda")
    opt = ops.Adam(m.parameters(), lr=1e-3)

    def fused(b):
        assert m.fused_train_step(*b, loss, opt)

    out["directau_fused_ms"] = _time(fused, batches, args.steps, args.warmup)

    tools.set_seed(2024)
    m2 = DirectAU(cfg, data, torch.device("cuda")).to("cuda")
    opt2 = ops.Adam(m2.parameters(), lr=1e-3)

    def autograd(b):
        ll = m2(*b)
        opt2.zero_grad()
        sum(ll).backward()
        opt2.step()

    out["directau_autograd_ms"] = _time(autograd, batches, max(args.steps // 5, 5), 3)

    tools.set_seed(2024)
    lg = LightGCN(dict(cfg, GCN_layer=cfg["GCN_layer"]), data, torch.device("cuda")).to("cuda")
    opt3 = ops.Adam(lg.parameters(), lr=1e-3)
    loss2 = torch.zeros(2, device="cuda")

    def lightgcn(b):
        assert lg.fused_train_step(*b, loss2, opt3)

    out["lightgcn_fused_ms"] = _time(lightgcn, batches, args.steps, args.warmup)
    out["directau_over_lightgcn"] = out["directau_fused_ms"] / out["lightgcn_fused_ms"]
    out["autograd_over_fused"] = out["directau_autograd_ms"] / out["directau_fused_ms"]
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in out.items()}))


if __name__ == "__main__":
    main()
