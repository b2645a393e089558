"""Fused, autograd-free training step of BIGCF (Zhang et al., SIGIR'24; reference: models/BIGCF.py:46-106 +
utility/utility_train/trainer.py:42-56) as a fixed chain of C-ABI calls on preallocated panels: a
PanelEngine (idgrec_amd/engine.py) whose InfoNCE id lists are planned as EgcfEngine's are.  d = 64, intent_size = 128.

Forward (n = U + I rows, users first; P = the packed [n, d] embedding panel, G = the symmetric normalised adjacency):
    X = G P + G^2 P + .. + G^K P                            idg_spmm_ex_f32, the running sum in the products' epilogues
                                                             (the SUM, not the mean; the ego layer is left out)
    T = softmax(X W) W^T,  F = X + T o Z                     idg_intent_fwd_f32, twice: user rows with W_u, item rows with W_i
    loss = BPR(F) + reg(P rows, W_u, W_i) + ssl_lambda (NCE(Fu, Fu) + NCE(Fp, Fp) + NCE(Fu, Fp) + NCE(Tu, Tu) + NCE(Tp, Tp))
over the RAW batch rows (duplicates count).  Z ~ N(0, 1) is the counter-based normal of (seed, stream, row, feature): it
is never stored, the backward regenerates it.

Backward.  The BPR scatter STORES gF at the batch's rows (its bitmap: users, positives, negatives) and the regulariser's
rows in GE; the self and the cross InfoNCE on F add into gF's rows; the self InfoNCE on T STORES gT at the user and positive
rows (a second bitmap of the slot: a negative's row has a gF but no gT, and what an earlier step left there is not read).
    (gF, gT, X) -> gX, [gW_u | gW_i]                         idg_intent_bwd_f32, twice, at the batch's bitmap; P is recomputed
    d loss / d P = G (gX + G (gX + ..)) + GE                 the Horner chain of masked products; the last one's epilogue
                                                             applies Adam to the embedding panel (K = 1: the one product
                                                             is the row-restricted launch, Adam follows on its own)
No dense panel is zeroed or restored: every reader of gF, gT, gX and GE is restricted to the batch's rows, so nothing an
earlier step left off them is seen (tests/test_gpu_bigcf.py runs two steps with different batches to hold that).

W_u and W_i are the two groups of PanelEngine's flat buffer, [W_u | W_i]: the two backward calls write their gradients
straight into their places, and the one Adam launch for both follows after the regulariser's reg_lambda W / d has joined the
gradient."""
import torch

from . import native, ops
from .engine import BatchPrep, PanelEngine, plan_infonce

lib = native.lib


class BigcfEngine(PanelEngine):
    def __init__(self, graph, num_users, num_items, params, intents, n_layers, reg_lambda=1e-4, ssl_lambda=0.2, temperature=0.2,
                 lr=1e-3, betas=(0.9, 0.999), eps=1e-8, store_grad=False):
        """params: the packed [n, 64] embedding panel (users first; updated in place).  intents: (W_u, W_i), [64, 128] each —
        copied into this engine's flat buffer; intent_views() returns the views to re-point the nn.Parameters at."""
        d, k = int(params.shape[1]), int(intents[0].shape[1])
        if (d, k) != (64, 128) or any(tuple(w.shape) != (d, k) for w in intents):
            raise ValueError("BigcfEngine: (embedding_size, intent_size) = (64, 128) only (got %s); other widths train through "
                             "the differentiable operators" % (tuple(intents[0].shape),))
        if int(n_layers) < 1:
            raise ValueError("BigcfEngine: GCN_layer >= 1 (the ego layer is not part of BIGCF's rows)")
        # two groups of one: [W_u | W_i].  loss: [bpr, reg_lambda * reg, ssl_lambda * (five InfoNCE terms)]
        super().__init__(graph, num_users, num_items, params, [(w,) for w in intents], 3, reg_lambda, lr, betas, eps, store_grad)
        self.K, self.k = int(n_layers), k
        self.ssl_lambda, self.temperature = float(ssl_lambda), float(temperature)
        n, dev = self.n, self.device
        f32 = dict(dtype=torch.float32, device=dev)
        self._W = tuple(g[0] for g in self._views)    # (W_u, W_i)
        self._GW = tuple(g[0] for g in self._gviews)  # their gradients
        panel = lambda: torch.empty((n, d), **f32)  # noqa: E731
        self.E = [panel() for _ in range(min(self.K - 1, 2))]  # layer ping-pong (K >= 2)
        self.S = panel() if self.K > 2 else None               # running layer sum (K >= 3)
        self.X, self.F, self.T = panel(), panel(), panel()
        self.GF, self.GT, self.GE, self.GX = panel(), panel(), panel(), panel()
        self.H = [panel() for _ in range(min(self.K - 1, 2))]  # the backward chain's ping-pong
        # the batch's row bitmap, its live units and scatter plan, the InfoNCE id lists and the (users, positives) bitmap:
        # side stream, one batch ahead
        self.prep = BatchPrep(self.U, n, d, dev, units_graph=graph, extra=self._plan_extra)
        self.ws = torch.empty(int(lib.idg_intent_bwd_workspace_bytes(d, k)), dtype=torch.uint8, device=dev)
        self._ssl = torch.zeros(6, **f32)  # F: user-user, pos-pos; T: user-user, pos-pos; F: user-pos (+ pad)
        self._wreg = torch.zeros(1, **f32)
        self._stream = None

    def intent_views(self):
        return self._W

    def intent_grads(self):
        return self._GW

    # ---- forward (every row): X, then (F, T) with the noise of `stream` = (seed, stream id), or of the panel `noise`
    @torch.no_grad()
    def forward(self, stream=None, noise=None):
        K, U, n = self.K, self.U, self.n
        prev, run = self.P, None
        for l in range(1, K + 1):
            last = l == K
            cur = None if last else self.E[(l - 1) & 1]
            if l == 1:
                ops.spmm_ex_raw(self.G, prev, Y=self.X if last else cur)
            else:
                ops.spmm_ex_raw(self.G, prev, Y=cur, sum_in=run, sum_out=self.X if last else self.S)
            run = cur if l == 1 else self.S
            prev = cur
        self._stream = stream if stream is not None else ops._next_noise_stream()
        seed, sid = self._stream
        for row0, nrows, w in ((0, U, self._W[0]), (U, n - U, self._W[1])):
            ops.intent_fwd_raw(self.X, w, self.T, self.F, row0=row0, nrows=nrows, noise=noise, seed=seed, stream_id=sid)
        return self.F, self.T

    # ---- one training step: losses [bpr, reg_lambda * reg, ssl_lambda * ssl]
    @torch.no_grad()
    def train_step(self, users, pos, neg, loss_out=None, stream=None, noise=None):
        n, d, K, U = self.n, self.d, self.K, self.U
        loss = self.loss if loss_out is None else loss_out
        slot = self.prep.take(users, pos, neg)
        bitmap = slot.bitmap
        self.forward(stream, noise)
        seed, sid = self._stream
        self._bpr(self.F, d, users, pos, neg, 1, loss, self.GF, slot)
        # the self-contrast terms: both arguments are the SAME rows, so the call takes one panel as both views and one
        # gradient panel as both gradients (idg_infonce_pair_f32 adds view 1's and view 2's rows into it, view 1 first)
        t, lam = self.temperature, self.ssl_lambda
        ops.infonce_pair_raw(self.F, self.F, users, pos, U, t, g1=self.GF, g2=self.GF, loss=self._ssl[0:2], dedup=False,
                             grad_scale=lam, accumulate=True, ws=slot.ssl_ws[0], planned=True)
        ops.infonce_cross_raw(self.F, users, pos, U, t, g=self.GF, loss=self._ssl[4:6], grad_scale=lam, ws=slot.ssl_ws[1],
                              planned=True)
        ops.infonce_pair_raw(self.T, self.T, users, pos, U, t, g1=self.GT, g2=self.GT, loss=self._ssl[2:4], dedup=False,
                             grad_scale=lam, accumulate=False, ws=slot.ssl_ws[0], planned=True)
        torch.sum(self._ssl[:5], dim=0, keepdim=True, out=loss[2:3])
        loss[2:3].mul_(lam)
        for i, (row0, nrows) in enumerate(((0, U), (U, n - U))):
            ops.intent_bwd_raw(self.GF, self.GT, bitmap, self.X, self._W[i], self.GX, self._GW[i], row0=row0, nrows=nrows,
                               noise=noise, seed=seed, stream_id=sid, ws=self.ws, gt_rows=slot.up_bitmap)
        # d loss / d P = G (gX + G (gX + ..)) + GE: gX lives on the batch's rows, the first product reads only those
        self.step_count += 1
        h, x_rows = self.GX, bitmap
        for l in range(1, K):
            nxt = self.H[(l - 1) & 1]
            ops.spmm_epi_raw(self.G, h, Y=nxt, addend=self.GX, mask=bitmap, x_rows=x_rows)
            h, x_rows = nxt, None
        adam = self._adam()
        if K == 1:
            # the only product reads gX, which exists at the batch's rows alone: the row-restricted launch, which has no Adam
            # epilogue — the finished gradient is stored and the dense Adam launch follows
            ops.spmm_epi_raw(self.G, h, Y=self.GRAD, addend=self.GE, mask=bitmap, x_rows=bitmap)
            ops.adam_step_raw(self.P, self.GRAD, *adam[1:])
        else:
            ops.spmm_epi_raw(self.G, h, addend=self.GE, mask=bitmap, sum_out=self.GRAD, adam=adam,
                             adam_discard_grad=not self.store_grad)
        # the intent matrices: reg_lambda * (1/2 ||W_u||^2 + 1/2 ||W_i||^2) / d joins loss[1], reg_lambda W / d the gradient
        c = self.reg_lambda / d
        self._wreg.copy_(torch.dot(self.SW, self.SW))
        loss[1:2].add_(self._wreg, alpha=0.5 * c)
        ops.lincomb_raw(self.SG, self.SG, 1.0, self.SW, c)
        self._adam_small()
        self.prep.release(slot)
        return loss

    def _plan_extra(self, slot, users, pos, neg, stream):
        """BatchPrep's hook: the id-list stages of the step's InfoNCE calls (raw user / item lists — shared by the self terms on
        F and on T — and the cross form), each into a workspace of the slot's own, and the bitmap of the user and positive
        rows (where gT lives)."""
        plan_infonce(slot, users, pos, self.U, self.n, self.d, self.device, stream)
        if getattr(slot, "up_bitmap", None) is None:
            slot.up_bitmap = torch.zeros((self.n + 31) // 32, dtype=torch.int32, device=self.device)
        ops.bpr_touch_rows_raw(users, pos, pos, self.U, slot.up_bitmap, stream=stream, clear_bits=self.n)
