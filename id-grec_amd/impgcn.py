"""Fused, autograd-free training step of IMP-GCN (Liu et al., WWW'21; reference: models/IMPGCN.py:50-108 +
utility/utility_train/trainer.py:42-56) as a fixed chain of C-ABI calls on preallocated panels: a PanelEngine
(idgrec_amd/engine.py), as GcmcEngine is.  d = 64, G = `group` in 1 .. 8, L = GCN_layer >= 1.

Forward (E0 = the packed [n, d] embedding panel, A = D^-1/2 Adj D^-1/2 without self loops, symmetric):
    side   = A . E0                                                       idg_spmm_f32 (the library's tuned product)
    member = groups of max(dropout(fc_group(dropout(leaky_relu(fc(E0 + side))))))      idg_group_assign_f32 (one byte per node;
             ties give several groups; item rows: every group)
    X_g^l  = A_g X_g^(l-1), l = 1 .. L-1, X_g^0 = E0, A_g = D_g A D_g;  S += sum_g X_g^l        idg_grouped_spmm_f32: ONE walk of
             the adjacency per l for all groups (the reference: G torch.sparse.mm calls per l)
    final  = (G E0 + S) / L                                               idg_lincomb_f32 (S_0 = G E0: the reference's quirk)
    loss   = BPR(final) + reg(user, positive and negative ego rows)       idg_bpr_fused_ex_f32 (reg_mode 1)

Backward.  The membership comes out of torch.eq(...).float(): no gradient reaches fc / fc_group, and final is LINEAR in E0
for the fixed membership.  With gF = d loss / d final (stored at the batch's rows only; what the panel holds elsewhere is
never read: the first product names the batch's bitmap as the live rows of its input, the later ones as those of the addend):
    H_g <- A_g gF;   H_g <- A_g (gF + H_g), L-1 grouped products in all;   Ssum = sum_g H_g  (the last product writes only it)
    d E0 = (1 / L) Ssum + at the batch's rows ((G / L) gF + the regulariser's rows)              idg_group_grad_f32
    Adam on the embedding panel                                                               idg_adam_step_f32
No forward panel is kept for the backward: it reads the membership bytes alone.  No dense panel is zeroed between steps;
tests/test_gpu_impgcn.py runs two steps with different batches to hold that.

The four small tensors (fc.weight, fc.bias, fc_group.weight, fc_group.bias: the reference's creation order) are ONE group of
PanelEngine's flat buffer, so the trainer's optimizer hand-off works as for the other engines; they take no gradient — in the
reference their .grad stays None and Adam skips them — so no Adam launch touches them: their values stay bit-unchanged and
their moments zero over any number of steps."""
import ctypes as C

import torch

from . import native, ops
from .engine import BatchPrep, PanelEngine

lib, check = native.lib, native.check


class ImpgcnEngine(PanelEngine):
    def __init__(self, graph, csr, num_users, num_items, params, small, n_layers, p=ops.IMPGCN_DROP, reg_lambda=1e-4, lr=1e-3,
                 betas=(0.9, 0.999), eps=1e-8, store_grad=False):
        """graph: the ops.Graph of the adjacency (side = A . E0); csr: the ops.GroupCsr of the same matrix.  params: the packed
        [n, 64] embedding panel (users first; updated in place).  small: (fc.weight [64, 64], fc.bias [64], fc_group.weight
        [G, 64], fc_group.bias [G]) — copied into this engine's flat buffer; small_views() returns the views to re-point the
        nn.Parameters at.  n_layers: GCN_layer (L - 1 products)."""
        d = int(params.shape[1])
        if d != 64:
            raise ValueError("ImpgcnEngine: d = 64 only (got %d); other widths train through the differentiable operators" % d)
        if len(small) != 4 or tuple(small[0].shape) != (d, d) or small[1].numel() != d or small[2].dim() != 2 or small[2].shape[1] != d \
                or small[3].numel() != small[2].shape[0]:
            raise ValueError("ImpgcnEngine: small must be (fc.weight [64, 64], fc.bias [64], fc_group.weight [G, 64], fc_group.bias [G])")
        G = ops._check_groups("ImpgcnEngine", small[2].shape[0])
        if int(n_layers) < 1:
            raise ValueError("ImpgcnEngine: GCN_layer >= 1 (got %d)" % int(n_layers))
        if not 0.0 <= float(p) < 1.0:
            raise ValueError("ImpgcnEngine: drop probability p = %g outside [0, 1)" % float(p))
        super().__init__(graph, num_users, num_items, params, [tuple(small)], 2, reg_lambda, lr, betas, eps, store_grad)
        if csr.n != self.n:
            raise ValueError("ImpgcnEngine: the CSR has %d rows, the panel %d" % (csr.n, self.n))
        self.csr, self.Gr, self.L, self.p = csr, G, int(n_layers), float(p)
        n, dev = self.n, self.device
        f32 = dict(dtype=torch.float32, device=dev)
        panel = lambda: torch.empty((n, d), **f32)  # noqa: E731
        self.SIDE, self.S, self.FINAL, self.GFIN, self.GE = panel(), panel(), panel(), panel(), panel()
        # X_g^l / H_g alternate between two grouped panels; rows outside a group's membership are never written nor read
        self.XG = [torch.empty((G, n, d), **f32) if self.L > 3 - k else None for k in range(2)]  # product l writes XG[l % 2]
        self.member = torch.empty(n, dtype=torch.uint8, device=dev)
        self.prep = BatchPrep(self.U, n, d, dev)  # the batch's row bitmap and scatter plan: side stream, one batch ahead
        self._streams = None

    def _products(self, X0, x_rows, V, v_rows, S, S_in):
        """The chain of L - 1 grouped products from the shared panel X0: Y_1 = A_g (X0), Y_l = A_g (Y_(l-1) + V).  accumulate
        (forward): every product adds its group sum into S; else (backward) only the last one writes S."""
        X, accumulate = X0, S_in is not False
        for l in range(1, self.L):
            last = l == self.L - 1
            Y = None if last else self.XG[l % 2]
            if accumulate:
                ops.grouped_spmm_raw(self.csr, self.member, X, self.Gr, Y=Y, S=S, S_in=None if l == 1 else S)
            elif l == 1:
                ops.grouped_spmm_raw(self.csr, self.member, X, self.Gr, Y=Y, S=S if last else None, x_rows=x_rows)
            else:
                ops.grouped_spmm_raw(self.csr, self.member, X, self.Gr, V=V, v_rows=v_rows, Y=Y, S=S if last else None)
            X = Y

    # ---- forward (every row); returns the [n, d] final panel
    @torch.no_grad()
    def forward(self, streams=None, training=True):
        """streams: ((seed, stream id) of the first mask, (seed, stream id) of the second) — one seed; default: the next two
        of the device seed's sequence.  training=False: both dropouts off (the evaluation panels)."""
        n, d, G, L, p_ = self.n, self.d, self.Gr, self.L, self._p
        st = ops._stream()
        if training and self.p > 0:
            self._streams = streams if streams is not None else (ops._next_noise_stream(), ops._next_noise_stream())
        else:
            self._streams = ((0, 0), (0, 0))
        (seed, s_fc), (seed2, s_grp) = self._streams
        if seed2 != seed:
            raise ValueError("ImpgcnEngine: the two masks share one seed (got %d and %d)" % (seed, seed2))
        wfc, bfc, wgrp, bgrp = self._views[0]
        self.G.spmm_raw(self.P, out=self.SIDE)
        check(lib.idg_group_assign_f32(p_(self.P), p_(self.SIDE), p_(wfc), p_(bfc), p_(wgrp), p_(bgrp), n, d, G, self.U, ops.IMPGCN_SLOPE,
                                       self.p if training else 0.0, C.c_uint64(seed), C.c_uint64(s_fc), C.c_uint64(s_grp),
                                       p_(self.member), None, st), "idg_group_assign_f32")
        if L > 1:
            self._products(self.P, None, None, None, self.S, None)
            ops.lincomb_raw(self.FINAL, self.P, G / L, self.S, 1.0 / L)
        else:
            ops.lincomb_raw(self.FINAL, self.P, float(G))
        return self.FINAL

    # ---- one training step: losses [bpr, reg_lambda * reg]
    @torch.no_grad()
    def train_step(self, users, pos, neg, loss_out=None, streams=None):
        n, d, G, L, p_ = self.n, self.d, self.Gr, self.L, self._p
        st = ops._stream()
        loss = self.loss if loss_out is None else loss_out
        slot = self.prep.take(users, pos, neg)
        bitmap = slot.bitmap
        self.forward(streams)
        self._bpr(self.FINAL, d, users, pos, neg, 1, loss, self.GFIN, slot)
        self.step_count += 1
        if L > 1:
            self._products(self.GFIN, bitmap, self.GFIN, bitmap, self.S, False)
        check(lib.idg_group_grad_f32(p_(self.S) if L > 1 else None, 1.0 / L, p_(self.GFIN), G / L, p_(self.GE), p_(bitmap), n, d,
                                     p_(self.GRAD), st), "idg_group_grad_f32")
        ops.adam_step_raw(self.P, self.GRAD, self.M, self.V, self.lr, self.step_count, self.betas[0], self.betas[1], self.eps)
        self.prep.release(slot)
        return loss
