"""Fused, autograd-free training step of MixRec (Zhang et al., WWW'25; reference: models/MixRec.py:44-60, 94-154 +
utility/utility_train/trainer.py:42-56) as a fixed chain of C-ABI calls on preallocated panels: a PanelEngine
(idgrec_amd/engine.py) without small tensors, its propagation and backward chain those of BigcfEngine.

Forward (n = U + I rows, users first; P = the packed [n, d] embedding panel, G = the symmetric normalised adjacency):
    X = G P + G^2 P + .. + G^K P                            idg_spmm_ex_f32, the running sum in the products' epilogues
                                                             (the SUM, not the mean; the ego layer is left out)
    loss = [item_beta BPR(X), (1 - item_beta) rect, reg_lambda reg(P rows), ssl_lambda (side_users + side_items)]
The host draws of the step — (user_beta, item_beta, nu [B], user_perm [B], item_perm [B]), draw_mix() — reach the device
through pinned staging and copies on the step's stream: no host synchronisation.

Backward.  idg_bpr_forward_f32 + idg_bpr_backward_f32 with the DEVICE scalars [item_beta, 1] as its upstream pair — the
weight on the BPR term, without a second BPR kernel — STORE gX at the batch's rows (the slot's bitmap) and the regulariser's
rows in GE; idg_mix_nce_f32 (csrc/idg_mixnce.hip) ADDS the gradients of the two contrastive entries into the same rows.
    d loss / d P = G (gX + G (gX + ..)) + GE                 the Horner chain of masked products; the last one's epilogue
                                                             applies Adam to the embedding panel (K = 1: the one product
                                                             is the row-restricted launch, Adam follows on its own)
No dense panel is zeroed or restored: every reader of gX and GE is restricted to the batch's rows."""
import numpy as np
import torch

from . import native, ops
from .engine import BatchPrep, PanelEngine

lib = native.lib


def draw_mix(B, alpha, beta, gamma):
    """The five host draws of one MixRec step, in the reference's order (models/MixRec.py:100-110) from numpy's and torch's
    GLOBAL generators: (user_beta, item_beta, nu float32 [B], user_perm int64 [B], item_perm int64 [B]).  A pure host
    function; seeded as the reference is, it returns the reference's stream."""
    user_beta = float(np.random.beta(alpha, beta))
    item_beta = float(np.random.beta(alpha, beta))
    nu = torch.FloatTensor(np.random.dirichlet([gamma] * int(B), 1)).reshape(-1)
    user_perm = torch.randperm(int(B))
    item_perm = torch.randperm(int(B))
    return user_beta, item_beta, nu, user_perm, item_perm


class _Stage:
    """Pinned host staging of one step's draws and their device copies: [user_perm | item_perm] int64 [2 B] and
    [item_beta, 1, 1, 1 | nu] float32 [4 + B] (the first four: the factors of the raw loss entries, whose first two are the
    BPR call's upstream pair).  `done` is recorded behind the copies; it is waited for only before the buffers are rewritten,
    several steps later."""

    def __init__(self, B, device):
        self.B = B
        self.h_idx = torch.empty(2 * B, dtype=torch.int64).pin_memory()
        self.h_f32 = torch.empty(4 + B, dtype=torch.float32).pin_memory()
        self.d_idx = torch.empty(2 * B, dtype=torch.int64, device=device)
        self.d_f32 = torch.empty(4 + B, dtype=torch.float32, device=device)
        self.done = None


class MixrecEngine(PanelEngine):
    STAGES = 4  # pinned staging buffers in rotation (the host stays at most two steps ahead of the device)

    def __init__(self, graph, num_users, num_items, params, n_layers, reg_lambda=1e-4, ssl_lambda=1.1, temperature=0.2, alpha=0.1,
                 beta=0.1, gamma=0.1, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, store_grad=False):
        """params: the packed [n, d] embedding panel (users first; updated in place), d one of the tiled SpMM widths."""
        d = int(params.shape[1])
        if d not in (32, 64, 128, 256):
            raise ValueError("MixrecEngine: d = %d (32, 64, 128, 256: the masked SpMM forms up to idg_mix_nce_f32's widest row); "
                             "other widths train through the differentiable operators" % d)
        if int(n_layers) < 1:
            raise ValueError("MixrecEngine: GCN_layer >= 1 (the ego layer is not part of MixRec's rows)")
        # loss: [item_beta bpr, (1 - item_beta) rect, reg_lambda reg, ssl_lambda (both sides)]
        super().__init__(graph, num_users, num_items, params, [], 4, reg_lambda, lr, betas, eps, store_grad)
        self.K = int(n_layers)
        self.ssl_lambda, self.temperature = float(ssl_lambda), float(temperature)
        self.alpha, self.beta, self.gamma = float(alpha), float(beta), float(gamma)
        n, dev = self.n, self.device
        f32 = dict(dtype=torch.float32, device=dev)
        panel = lambda: torch.empty((n, d), **f32)  # noqa: E731
        self.E = [panel() for _ in range(min(self.K - 1, 2))]  # layer ping-pong (K >= 2)
        self.S = panel() if self.K > 2 else None               # running layer sum (K >= 3)
        self.X, self.GX, self.GE = panel(), panel(), panel()
        self.H = [panel() for _ in range(min(self.K - 1, 2))]  # the backward chain's ping-pong
        self.prep = BatchPrep(self.U, n, d, dev, units_graph=graph)
        self._raw = torch.zeros(4, **f32)  # [bpr, reg_lambda reg, (1 - item_beta) rect, ssl_lambda ssl] as the kernels leave them
        self._scaled = torch.zeros(4, **f32)
        self._order = torch.tensor([0, 2, 1, 3], dtype=torch.int64, device=dev)
        self._stages, self._stage_no = {}, 0
        self._mix_ws = {}

    # ---- forward (every row): X
    @torch.no_grad()
    def forward(self):
        K = self.K
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
        return self.X

    def _stage(self, B, draws):
        """The draws on the device: (user_perm, item_perm, nu, factors [4]) views of the stage's device buffers."""
        ring = self._stages.setdefault(B, [])
        self._stage_no += 1
        i = self._stage_no % self.STAGES
        while len(ring) <= i:
            ring.append(_Stage(B, self.device))
        st = ring[i]
        if st.done is not None:
            st.done.synchronize()  # the copies of STAGES steps ago: long complete
        _, item_beta, nu, user_perm, item_perm = draws
        st.h_idx[:B].copy_(user_perm)
        st.h_idx[B:].copy_(item_perm)
        st.h_f32[0] = item_beta
        st.h_f32[1:4] = 1.0
        st.h_f32[4:].copy_(nu)
        st.d_idx.copy_(st.h_idx, non_blocking=True)
        st.d_f32.copy_(st.h_f32, non_blocking=True)
        if st.done is None:
            st.done = torch.cuda.Event()
        st.done.record()
        return st.d_idx[:B], st.d_idx[B:], st.d_f32[4:], st.d_f32[:4]

    # ---- one training step: losses [item_beta bpr, (1 - item_beta) rect, reg_lambda reg, ssl_lambda ssl]
    @torch.no_grad()
    def train_step(self, users, pos, neg, loss_out=None, draws=None):
        """draws: (user_beta, item_beta, nu, user_perm, item_perm) host values (default: draw_mix)."""
        n, d, K, U, p_ = self.n, self.d, self.K, self.U, self._p
        B = int(users.shape[0])
        loss = self.loss if loss_out is None else loss_out
        if draws is None:
            draws = draw_mix(B, self.alpha, self.beta, self.gamma)
        user_beta, item_beta = float(draws[0]), float(draws[1])
        slot = self.prep.take(users, pos, neg)
        bitmap = slot.bitmap
        user_perm, item_perm, nu, factors = self._stage(B, draws)
        self.forward()
        st = ops._stream()
        args = (p_(self.X), p_(self.P), U, n, p_(users), p_(pos), p_(neg), B, d, self.reg_lambda)
        native.check(lib.idg_bpr_forward_f32(*args, p_(self._raw), p_(slot.ws), st), "idg_bpr_forward_f32")
        native.check(lib.idg_bpr_backward_f32(*args, p_(factors), p_(self.GX), p_(self.GE),
                                              native.IDG_BPR_PLANNED | native.IDG_BPR_TOUCHED_PRESET, p_(bitmap), p_(slot.ws), st),
                     "idg_bpr_backward_f32")
        ws = self._mix_ws.get(B)
        if ws is None:
            ws = self._mix_ws[B] = ops.mix_nce_workspace(B, d, self.device)
        ops.mix_nce_raw(self.X, U, users, pos, neg, user_perm, item_perm, nu, user_beta, item_beta, self.temperature,
                        self.ssl_lambda, loss=self._raw[2:4], g_panel=self.GX, ws=ws)
        torch.mul(self._raw, factors, out=self._scaled)
        torch.index_select(self._scaled, 0, self._order, out=loss)
        # d loss / d P = G (gX + G (gX + ..)) + GE: gX lives on the batch's rows, the first product reads only those
        self.step_count += 1
        h, x_rows = self.GX, bitmap
        for l in range(1, K):
            nxt = self.H[(l - 1) & 1]
            ops.spmm_epi_raw(self.G, h, Y=nxt, addend=self.GX, mask=bitmap, x_rows=x_rows)
            h, x_rows = nxt, None
        adam = self._adam()
        if K == 1:
            ops.spmm_epi_raw(self.G, h, Y=self.GRAD, addend=self.GE, mask=bitmap, x_rows=bitmap)
            ops.adam_step_raw(self.P, self.GRAD, *adam[1:])
        else:
            ops.spmm_epi_raw(self.G, h, addend=self.GE, mask=bitmap, sum_out=self.GRAD, adam=adam,
                             adam_discard_grad=not self.store_grad)
        self.prep.release(slot)
        return loss
