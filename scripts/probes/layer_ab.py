"""The d = 64 layer kernels on fixed inputs: forward and backward of the NGCF, LR-GCCF, GCMC, BIGCF (intent) and IMP-GCN
(group assignment) layer entry points and idg_linear_wgrad_f32, n = 8257, both (seed, stream) pairs of the tests, a 5 % row
bitmap, gN read from a slot of a wider panel.  Prints a checksum of the raw bits of every output.
Run once with the working tree's library and once with IDG_LIB_PATH=<other build>: equal lines = bit-identical."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

from idgrec_amd import native, ops
from tests.test_gpu_ngcf import SLOPE, STREAMS, _bitmap, _ok, _p

lib = native.lib
n, d, k, G, LD, SLOT, P = 8257, 64, 128, 3, 256, 128, 0.1
rng = np.random.default_rng(20)
randn = lambda *shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).cuda()  # noqa: E731
zeros = lambda *shape: torch.zeros(shape, device="cuda")  # noqa: E731
side, ego, gE = randn(n, d), randn(n, d), randn(n, d)
W1, W2, b1, b2 = randn(d, d) * 0.1, randn(d, d) * 0.1, randn(d) * 0.1, randn(d) * 0.1
Wk, Wgrp, bgrp = randn(d, k) * 0.1, randn(G, d), randn(G)
rows = np.sort(rng.choice(n, n // 20, replace=False))
bitmap = _bitmap(n, rows)
gpanel = torch.full((n, LD), float("nan"), device="cuda")  # gN lives in one slot, at the flagged rows only
gpanel[torch.from_numpy(rows).cuda(), SLOT:SLOT + d] = randn(len(rows), d)
st = ops._stream()


def ws_of(name, *a):
    return torch.empty(max(int(getattr(lib, name)(*a)), 16), dtype=torch.uint8, device="cuda")


def show(name, stream, *outs):
    torch.cuda.synchronize()
    sums = " ".join(hashlib.sha1(t.detach().cpu().numpy().tobytes()).hexdigest()[:12] for t in outs)
    print("%-14s seed %-11d %s" % (name, stream[0], sums), flush=True)


for stream in STREAMS:
    seed, sid = stream
    # NGCF
    E, N, gs, gg, wg = zeros(n, d), zeros(n, LD), zeros(n, d), zeros(n, d), zeros(2 * d * d + 2 * d)
    _ok(lib.idg_ngcf_layer_fwd_f32(_p(side), _p(ego), _p(W1), _p(W2), _p(b1), _p(b2), n, d, SLOPE, P, seed, sid, _p(E), _p(N, SLOT), LD,
                                   st), "idg_ngcf_layer_fwd_f32")
    show("ngcf fwd", stream, E, N)
    _ok(lib.idg_ngcf_layer_bwd_f32(_p(E), _p(gE), _p(gpanel, SLOT), LD, _p(bitmap), _p(side), _p(ego), _p(W1), _p(W2), n, d, SLOPE, P,
                                   seed, sid, _p(gs), _p(gg), _p(wg), _p(ws_of("idg_ngcf_layer_bwd_workspace_bytes", d)), st),
        "idg_ngcf_layer_bwd_f32")
    show("ngcf bwd", stream, gs, gg, wg)
    # LR-GCCF
    E, gs, wg = zeros(n, LD), zeros(n, d), zeros(d * d + d)
    ops.gccf_layer_fwd_raw(side, W1, b1, P, seed, sid, E, slot=SLOT)
    show("gccf fwd", stream, E)
    ops.gccf_layer_bwd_raw(gE, gpanel, LD, bitmap, side, W1, P, seed, sid, gs, wg, gn_slot=SLOT)
    show("gccf bwd", stream, gs, wg)
    # GCMC
    T, N, gs, wg = zeros(n, d), zeros(n, LD), zeros(n, d), zeros(2 * (d * d + d))
    ops.gcmc_layer_fwd_raw(side, W1, b1, W2, b2, P, seed, sid, T, N, slot=SLOT)
    show("gcmc fwd", stream, T, N)
    ops.gcmc_layer_bwd_raw(T, gE, gpanel, LD, bitmap, side, W1, b1, W2, P, seed, sid, gs, wg, gn_slot=SLOT)
    show("gcmc bwd", stream, gs, wg)
    # BIGCF's intent layer: every row, then the flagged rows with gT_in at its own bitmap
    for name, bits in (("intent", None), ("intent rows", bitmap)):
        T, F, gX, gW = zeros(n, d), zeros(n, d), zeros(n, d), zeros(d, k)
        ops.intent_fwd_raw(side, Wk, T, F, rows_bitmap=bits, seed=seed, stream_id=sid)
        show(name + " fwd", stream, T, F)
        ops.intent_bwd_raw(gE, gpanel[:, SLOT:SLOT + d], bits, side, Wk, gX, gW, seed=seed, stream_id=sid, gt_rows=bitmap)
        show(name + " bwd", stream, gX, gW)
    # IMP-GCN's group assignment
    scores = zeros(n, G)
    member = ops.group_assign_raw(ego, side, W1, b1, Wgrp, bgrp, n // 2, P, seed, sid, sid + 1, scores_out=scores)
    show("group assign", stream, member, scores)
    # the dense weight gradient: written, then accumulated into
    wgrad = ops.linear_wgrad_raw(side, gE)
    ops.linear_wgrad_raw(ego, gE, out=wgrad, accumulate=True)
    show("linear wgrad", stream, wgrad)
