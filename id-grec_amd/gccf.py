"""Fused, autograd-free training step of LR-GCCF (Chen et al., AAAI'20; reference: models/GCCF.py:60-110 +
utility/utility_train/trainer.py:42-56) as a fixed chain of C-ABI calls on preallocated panels, in the pattern of
idgrec_amd/ngcf.py.  d = 64, every layer d -> d, node dropout off.

Forward, layer l = 1..K (E_0 = the packed [n, d] embedding panel, G = D^-1/2 (A + I) D^-1/2):
    side_l = G . E_{l-1}                                   idg_spmm_f32
    E_l    = dropout(side_l . W_l + b_l)                   idg_gccf_layer_fwd_f32, written INTO slot l of the concatenated
                                                           final rows [n, (K+1) d] (models/GCCF.py:88)
    loss   = BPR(final) + reg(item rows only)              idg_bpr_fused_ex_f32 (final width (K+1) d, ego width d)
E_l lives ONLY in its slot: the next layer's product reads it from there (idg_spmm_f32 takes the leading dimension of its
input; Graph.spmm_raw passes a column slice through), so no contiguous copy of a layer is kept.

Backward, l = K..1, with gN_l = slot l of d loss / d final (stored at the batch's rows only):
    gT = keep * (gE_l + gN_l);  gb_l = column sums of gT;  gW_l = side_l^T gT;  g_side = gT . W_l^T     idg_gccf_layer_bwd_f32
    gE_{l-1} = G . g_side   (G symmetric; this model has no g_ego term)
No activation is saved or read: the layer is linear between the mask and the product, and the mask is a function of
(seed, stream, row, feature).  For l = 1 the gradient of slot 0 (E_0 is itself part of the final rows) and the
regulariser's rows join G . g_side in the product whose epilogue applies Adam to the embedding panel.  NGCF adds those rows
into its dense g_ego panel; here no dense panel exists, and none is zeroed or restored: the regulariser's gradient panel GE
— which the loss kernel stores (not accumulates) at every row of the batch, a zero row for users — receives slot 0's rows
at the batch's rows (idg_rows_add2_f32), and the product takes it as an addend MASKED by the batch's bitmap
(idg_epilogue.mask: rows whose bit is clear count as zero and are not read).  What an earlier step left in GE off this
step's rows is therefore never seen; tests/test_gpu_gccf.py runs two steps with different batches to hold that.

The 2K small tensors live in ONE flat buffer [W_1 | b_1 | W_2 | b_2 | ...] (views handed back to the nn.Parameters), as do
their gradients — idg_gccf_layer_bwd_f32 writes [gW | gb] straight into the layer's place — and both Adam moments: one
Adam launch for all of them."""
import ctypes as C

import torch

from . import native, ops
from .engine import BatchPrep

lib, check = native.lib, native.check


class GccfEngine:
    def __init__(self, graph, num_users, num_items, params, small, mess_dropout=(0.1, 0.1, 0.1), reg_lambda=1e-4, lr=1e-4,
                 betas=(0.9, 0.999), eps=1e-8, store_grad=False):
        """params: the packed [n, 64] embedding panel (users first; updated in place).  small: K tuples (W_gcn [d, d],
        b_gcn [1, d]) of tensors — copied into this engine's flat buffer; small_views() returns the views to re-point the
        nn.Parameters at."""
        self.G = graph
        self.U, self.I = int(num_users), int(num_items)
        self.n, self.d = int(params.shape[0]), int(params.shape[1])
        self.K = len(small)
        assert self.n == self.U + self.I and params.is_cuda and params.is_contiguous()
        d, n, K = self.d, self.n, self.K
        if d != 64:
            raise ValueError("GccfEngine: d = 64 only (got %d); other widths train through the differentiable operators" % d)
        if K < 1 or len(mess_dropout) < K:
            raise ValueError("GccfEngine: K >= 1 layers and one drop probability per layer")
        for t in small:
            if tuple(t[0].shape) != (d, d) or t[1].numel() != d:
                raise ValueError("GccfEngine: every layer must map d -> d (layer_size = [d] * K)")
        self.D = (K + 1) * d
        self.p = [float(x) for x in mess_dropout]
        self.reg_lambda, self.lr, self.betas, self.eps = float(reg_lambda), float(lr), betas, float(eps)
        self.store_grad = bool(store_grad)
        dev = params.device
        self.device = dev
        f32 = dict(dtype=torch.float32, device=dev)
        self.P = params
        per = self._per = d * d + d
        self.SW, self.SG = torch.empty(K * per, **f32), torch.zeros(K * per, **f32)
        self.SM, self.SV = torch.zeros(K * per, **f32), torch.zeros(K * per, **f32)
        self._views, self._gviews = [], []
        for l, (w, b) in enumerate(small):
            o = l * per
            cuts = [(o, (d, d)), (o + d * d, (1, d))]
            vs = [self.SW[a:a + s[0] * s[1]].view(s) for a, s in cuts]
            vs[0].copy_(w)
            vs[1].copy_(b.reshape(1, d))
            self._views.append(tuple(vs))
            self._gviews.append(tuple(self.SG[a:a + s[0] * s[1]].view(s) for a, s in cuts))
        panel = lambda: torch.empty((n, d), **f32)  # noqa: E731
        self.SIDE = [panel() for _ in range(K)]
        self.FINAL = torch.empty((n, self.D), **f32)
        self.GFIN = torch.empty((n, self.D), **f32)
        self.GE = panel()       # the regulariser's rows, then + slot 0's rows: the masked addend of the last product
        self.gE = panel()       # d loss / d E_l as the next layer's input
        self.g_side = panel()
        self.GRAD = panel()
        self.M, self.V = torch.zeros((n, d), **f32), torch.zeros((n, d), **f32)
        self.prep = BatchPrep(self.U, n, d, dev)  # the batch's row bitmap and scatter plan: side stream, one batch ahead
        self.ws = torch.empty(int(lib.idg_gccf_layer_bwd_workspace_bytes(d)), dtype=torch.uint8, device=dev)
        self.loss = torch.zeros(2, **f32)
        self.step_count = 0
        self._streams = None

    def small_views(self):
        return self._views

    def small_grads(self):
        return self._gviews

    @staticmethod
    def _p(t):
        return None if t is None else C.c_void_p(t.data_ptr())

    def layer(self, l):
        """E_l: slot l of the final panel (l = 0: the copy of the embedding panel)."""
        return self.FINAL[:, l * self.d:(l + 1) * self.d]

    # ---- forward (every row); returns the [n, (K+1) d] final panel
    @torch.no_grad()
    def forward(self, streams=None):
        n, d, D, K, p_ = self.n, self.d, self.D, self.K, self._p
        st = ops._stream()
        self._streams = streams if streams is not None else [ops._next_noise_stream() for _ in range(K)]
        check(lib.idg_copy_cols_f32(p_(self.FINAL), D, p_(self.P), d, n, d, st), "idg_copy_cols_f32")
        for l in range(K):
            w, b = self._views[l]
            self.G.spmm_raw(self.P if l == 0 else self.layer(l), out=self.SIDE[l])
            seed, sid = self._streams[l]
            slot = C.c_void_p(self.FINAL.data_ptr() + 4 * (l + 1) * d)
            check(lib.idg_gccf_layer_fwd_f32(p_(self.SIDE[l]), p_(w), p_(b), n, d, self.p[l], C.c_uint64(seed), C.c_uint64(sid),
                                             slot, D, st), "idg_gccf_layer_fwd_f32")
        return self.FINAL

    # ---- one training step: losses [bpr, reg_lambda * reg]
    @torch.no_grad()
    def train_step(self, users, pos, neg, loss_out=None, streams=None):
        n, d, D, K, U, p_ = self.n, self.d, self.D, self.K, self.U, self._p
        st = ops._stream()
        B = int(users.shape[0])
        loss = self.loss if loss_out is None else loss_out
        slot = self.prep.take(users, pos, neg)
        bitmap = slot.bitmap
        self.forward(streams)
        check(lib.idg_bpr_fused_ex_f32(p_(self.FINAL), D, p_(self.P), d, U, n, p_(users), p_(pos), p_(neg), B, self.reg_lambda, 0,
                                       p_(loss), p_(self.GFIN), p_(self.GE), native.IDG_BPR_PLANNED | native.IDG_BPR_TOUCHED_PRESET,
                                       p_(bitmap), p_(slot.ws), st), "idg_bpr_fused_ex_f32")
        self.step_count += 1
        gE = None
        for l in range(K - 1, -1, -1):
            w, _ = self._views[l]
            seed, sid = self._streams[l]
            gN = C.c_void_p(self.GFIN.data_ptr() + 4 * (l + 1) * d)
            w_grads = C.c_void_p(self.SG.data_ptr() + 4 * l * self._per)  # [gW | gb] straight into the flat buffer
            check(lib.idg_gccf_layer_bwd_f32(p_(gE), gN, D, p_(bitmap), p_(self.SIDE[l]), p_(w), n, d, self.p[l], C.c_uint64(seed),
                                             C.c_uint64(sid), p_(self.g_side), w_grads, p_(self.ws), st), "idg_gccf_layer_bwd_f32")
            if l > 0:
                gE = self.G.spmm_raw(self.g_side, out=self.gE)  # the backward of side = G . E: G^T . g_side, G symmetric
            else:
                # GE (the regulariser's rows, stored at the batch's rows) += slot 0's rows; the product reads GE at those
                # rows only (mask) and its epilogue applies Adam to the embedding panel
                check(lib.idg_rows_add2_f32(p_(self.GE), d, p_(self.GFIN), D, None, 0, p_(bitmap), n, d, st), "idg_rows_add2_f32")
                ops.spmm_epi_raw(self.G, self.g_side, addend=self.GE, mask=bitmap, sum_out=self.GRAD,
                                 adam=(self.P, self.M, self.V, self.lr, self.step_count, self.betas[0], self.betas[1], self.eps),
                                 adam_discard_grad=not self.store_grad)
        ops.adam_step_raw(self.SW, self.SG, self.SM, self.SV, self.lr, self.step_count, self.betas[0], self.betas[1], self.eps)
        self.prep.release(slot)
        return loss

    def prefetch(self, users, pos, neg):
        """One-batch lookahead of the index-only work of the NEXT step (side stream)."""
        self.prep.prefetch(users, pos, neg)
