"""Fused, autograd-free training step of GCMC (reference: models/GCMC.py:66-116 + utility/utility_train/trainer.py:42-56) as a
fixed chain of C-ABI calls on preallocated panels: a PanelEngine (idgrec_amd/engine.py), as GccfEngine is.  d = 64, every
layer d -> d; the model has no node dropout.

Forward, layer l = 1..K (T_0 = the packed [n, d] embedding panel, G = D^-1/2 A D^-1/2 without self loops):
    side_l    = G . T_{l-1}                                            idg_spmm_f32
    T_l, N_l  = the layer kernel: T = dropout(leaky_relu(side . W_gcn + b_gcn) . W_mlp + b_mlp), N = normalize(T)
                                                                       idg_gcmc_layer_fwd_f32
                T_l contiguous (the next product's input, un-normalised); N_l INTO slot l of the concatenated final rows
                [n, (K+1) d] (models/GCMC.py:88-92); slot 0 is the copy of the embedding panel
    loss      = BPR(final) + reg(user, positive and negative ego rows)  idg_bpr_fused_ex_f32 (reg_mode 1)

Backward, l = K..1, with gN_l = slot l of d loss / d final (stored at the batch's rows only) and gE_l = d loss / d T_l as the
next layer's input (none at l = K):
    g_side, [gW_gcn | gb_gcn | gW_mlp | gb_mlp]                        idg_gcmc_layer_bwd_f32 (reads T_l and side_l;
                                                                       H and A recomputed, never stored)
    gE_{l-1} = G . g_side   (G symmetric)
For l = 1 the gradient of slot 0 and the regulariser's rows join G . g_side in the product whose epilogue applies Adam to the
embedding panel — GccfEngine's scheme: the regulariser's panel GE, stored (not accumulated) at every row of the batch by the
loss kernel, receives slot 0's rows at the batch's rows (idg_rows_add2_f32) and is the product's addend MASKED by the batch's
bitmap.  No dense panel is zeroed or restored; tests/test_gpu_gcmc.py runs two steps with different batches to hold that.

The 4K small tensors are the groups (W_gcn_l, b_gcn_l, W_mlp_l, b_mlp_l) of PanelEngine's flat buffer, the reference's
creation order: idg_gcmc_layer_bwd_f32 writes its four gradients straight into the layer's place of the gradient buffer."""
import ctypes as C

import torch

from . import native, ops
from .engine import BatchPrep, PanelEngine

lib, check = native.lib, native.check


class GcmcEngine(PanelEngine):
    def __init__(self, graph, num_users, num_items, params, small, mess_dropout=(0.1, 0.1, 0.1), reg_lambda=1e-4, lr=1e-4,
                 betas=(0.9, 0.999), eps=1e-8, store_grad=False):
        """params: the packed [n, 64] embedding panel (users first; updated in place).  small: K tuples (W_gcn [d, d],
        b_gcn [1, d], W_mlp [d, d], b_mlp [1, d]) of tensors — copied into this engine's flat buffer; small_views() returns the
        views to re-point the nn.Parameters at."""
        d, K = int(params.shape[1]), len(small)
        if d != 64:
            raise ValueError("GcmcEngine: d = 64 only (got %d); other widths train through the differentiable operators" % d)
        if K < 1 or len(mess_dropout) < K:
            raise ValueError("GcmcEngine: K >= 1 layers and one drop probability per layer")
        for t in small:
            if len(t) != 4 or tuple(t[0].shape) != (d, d) or t[1].numel() != d or tuple(t[2].shape) != (d, d) or t[3].numel() != d:
                raise ValueError("GcmcEngine: every layer must map d -> d (layer_size = [d] * K)")
        super().__init__(graph, num_users, num_items, params,
                         [(wg, bg.reshape(1, d), wm, bm.reshape(1, d)) for wg, bg, wm, bm in small], 2, reg_lambda, lr, betas, eps,
                         store_grad)
        self.K = K
        n, dev = self.n, self.device
        self.D = (K + 1) * d
        self.p = [float(x) for x in mess_dropout]
        self.slope = ops.GCMC_SLOPE
        f32 = dict(dtype=torch.float32, device=dev)
        panel = lambda: torch.empty((n, d), **f32)  # noqa: E731
        self.SIDE = [panel() for _ in range(K)]
        self.T = [panel() for _ in range(K)]  # T_l: the next product's input and what the layer's backward reads
        self.FINAL = torch.empty((n, self.D), **f32)
        self.GFIN = torch.empty((n, self.D), **f32)
        self.GE = panel()       # the regulariser's rows, then + slot 0's rows: the masked addend of the last product
        self.gE = panel()       # d loss / d T_l as the next layer's input
        self.g_side = panel()
        self.prep = BatchPrep(self.U, n, d, dev)  # the batch's row bitmap and scatter plan: side stream, one batch ahead
        self.ws = torch.empty(int(lib.idg_gcmc_layer_bwd_workspace_bytes(d)), dtype=torch.uint8, device=dev)
        self._streams = None

    def layer(self, l):
        """Slot l of the final panel: N_l (l = 0: the copy of the embedding panel)."""
        return self.FINAL[:, l * self.d:(l + 1) * self.d]

    # ---- forward (every row); returns the [n, (K+1) d] final panel
    @torch.no_grad()
    def forward(self, streams=None):
        n, d, D, K, p_ = self.n, self.d, self.D, self.K, self._p
        st = ops._stream()
        self._streams = streams if streams is not None else [ops._next_noise_stream() for _ in range(K)]
        check(lib.idg_copy_cols_f32(p_(self.FINAL), D, p_(self.P), d, n, d, st), "idg_copy_cols_f32")
        for l in range(K):
            wg, bg, wm, bm = self._views[l]
            self.G.spmm_raw(self.P if l == 0 else self.T[l - 1], out=self.SIDE[l])
            seed, sid = self._streams[l]
            slot = C.c_void_p(self.FINAL.data_ptr() + 4 * (l + 1) * d)
            check(lib.idg_gcmc_layer_fwd_f32(p_(self.SIDE[l]), p_(wg), p_(bg), p_(wm), p_(bm), n, d, self.slope, self.p[l],
                                             C.c_uint64(seed), C.c_uint64(sid), p_(self.T[l]), slot, D, st), "idg_gcmc_layer_fwd_f32")
        return self.FINAL

    # ---- one training step: losses [bpr, reg_lambda * reg]
    @torch.no_grad()
    def train_step(self, users, pos, neg, loss_out=None, streams=None):
        n, d, D, K, p_ = self.n, self.d, self.D, self.K, self._p
        st = ops._stream()
        loss = self.loss if loss_out is None else loss_out
        slot = self.prep.take(users, pos, neg)
        bitmap = slot.bitmap
        self.forward(streams)
        self._bpr(self.FINAL, D, users, pos, neg, 1, loss, self.GFIN, slot)
        self.step_count += 1
        gE = None
        for l in range(K - 1, -1, -1):
            wg, bg, wm, _ = self._views[l]
            seed, sid = self._streams[l]
            gN = C.c_void_p(self.GFIN.data_ptr() + 4 * (l + 1) * d)
            w_grads = C.c_void_p(self.SG.data_ptr() + 4 * self.group_offset[l])  # the four gradients straight into the flat buffer
            check(lib.idg_gcmc_layer_bwd_f32(p_(self.T[l]), p_(gE), gN, D, p_(bitmap), p_(self.SIDE[l]), p_(wg), p_(bg), p_(wm), n, d,
                                             self.slope, self.p[l], C.c_uint64(seed), C.c_uint64(sid), p_(self.g_side), w_grads,
                                             p_(self.ws), st), "idg_gcmc_layer_bwd_f32")
            if l > 0:
                gE = self.G.spmm_raw(self.g_side, out=self.gE)  # the backward of side = G . T: G^T . g_side, G symmetric
            else:
                # GE (the regulariser's rows, stored at the batch's rows) += slot 0's rows; the product reads GE at those
                # rows only (mask) and its epilogue applies Adam to the embedding panel
                check(lib.idg_rows_add2_f32(p_(self.GE), d, p_(self.GFIN), D, None, 0, p_(bitmap), n, d, st), "idg_rows_add2_f32")
                ops.spmm_epi_raw(self.G, self.g_side, addend=self.GE, mask=bitmap, sum_out=self.GRAD, adam=self._adam(),
                                 adam_discard_grad=not self.store_grad)
        self._adam_small()
        self.prep.release(slot)
        return loss
