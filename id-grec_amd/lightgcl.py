"""Fused, autograd-free training step of LightGCL (Cai et al., ICLR'23; reference: models/LightGCL.py:58-124 +
utility/utility_train/trainer.py:42-56) as a fixed chain of C-ABI calls on preallocated panels: a PanelEngine
(idgrec_amd/engine.py) without small tensors.

Forward (n = U + I rows, users first; P = the packed [n, d] embedding panel, G = the symmetric normalised adjacency, whose
off-diagonal block is the reference's rectangular D_u^-1/2 R D_i^-1/2: its pair R E_i, R^T E_u per hop is ONE product):
    F = P + G P + .. + G^K P                                idg_spmm_ex_f32, the running sum in the products' epilogues
    T = F - G^K P = the sum of the layers below K           idg_lincomb_f32
    P_i = V^T T_i,  P_u = U^T T_u                           idg_lowrank_project_f32 (two [q, d] results)
The reference's SVD view, summed over its layers, is G_u = P_u-rows + (U S) P_i and G_i = P_i-rows + (V S) P_u by linearity;
only the batch's rows are read, and idg_svd_nce_f32 (csrc/idg_svdnce.hip) forms them in its operand packing.
    loss = [bpr(F), reg_lambda reg(P rows), ssl_lambda (lse_u + lse_i - pos_u - pos_i)]

Backward.  idg_bpr_forward_f32 + idg_bpr_backward_f32 ADD gF at the batch's rows and the regulariser's rows into GE (both
zeroed: the contrastive terms are dense); two idg_svd_nce_f32 calls with the device pair [ssl_lambda, -ssl_lambda] as their
upstream ADD the table gradients into all rows of gF, gQ into the batch's rows of GE, and deliver dP_i, dP_u; two
idg_lowrank_expand_f32 calls STORE gT_i = V dP_i and gT_u = U dP_u.  With d loss / d E^K = gF and d loss / d E^l = gF + gT
below K:
    g_K = gF,   g_k = G g_(k+1) + gF + gT (k < K),   d loss / d P = g_0 + GE
and a dense Adam step of the packed panel: the table terms reach every row, as in LayerChainRecommender.fused_train_step."""
import torch

from . import ops
from .engine import PanelEngine


class LightgclEngine(PanelEngine):
    def __init__(self, graph, num_users, num_items, params, n_layers, svd_u, s, svd_v, reg_lambda=1e-6, ssl_lambda=0.5,
                 temperature=0.2, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, store_grad=False):
        """params: the packed [n, d] embedding panel (users first; updated in place), d one of the tiled SpMM widths.
        svd_u [U, q], s [q], svd_v [I, q]: the factors of a truncated SVD of the rectangular normalised adjacency — inputs;
        the engine never computes them."""
        d = int(params.shape[1])
        if d not in (32, 64, 128, 256):
            raise ValueError("LightgclEngine: d = %d (32, 64, 128, 256: the tiled SpMM widths up to idg_svd_nce_f32's widest row); "
                             "other widths train through the differentiable operators" % d)
        if int(n_layers) < 1:
            raise ValueError("LightgclEngine: GCN_layer >= 1 (the SVD view is built from the layers below the last)")
        super().__init__(graph, num_users, num_items, params, [], 3, reg_lambda, lr, betas, eps, store_grad)
        n, dev, U, I = self.n, self.device, self.U, self.I
        f32 = dict(dtype=torch.float32, device=dev)
        q = int(s.shape[0])
        if tuple(svd_u.shape) != (U, q) or tuple(svd_v.shape) != (I, q) or not 1 <= q <= ops.LOWRANK_MAX_RANK:
            raise ValueError("LightgclEngine: factors %s, %s, %s for %d users and %d items (rank 1 .. %d)"
                             % (tuple(svd_u.shape), tuple(s.shape), tuple(svd_v.shape), U, I, ops.LOWRANK_MAX_RANK))
        self.K, self.q = int(n_layers), q
        self.ssl_lambda, self.temperature = float(ssl_lambda), float(temperature)
        self.svd_u = svd_u.detach().to(**f32).contiguous()
        self.svd_v = svd_v.detach().to(**f32).contiguous()
        s = s.detach().to(**f32)
        self.us, self.vs = (self.svd_u * s).contiguous(), (self.svd_v * s).contiguous()
        panel = lambda: torch.empty((n, d), **f32)  # noqa: E731
        self.E = [panel() for _ in range(min(self.K, 2))]  # layer ping-pong; E^K stays in E[(K - 1) & 1]
        self.S = panel() if self.K > 1 else None           # running layer sum below the last layer
        self.F, self.T = panel(), panel()
        self.GF, self.GE, self.GT = panel(), panel(), panel()
        self.H = [panel() for _ in range(min(self.K - 1, 2))]  # the backward chain's ping-pong
        self.Pi, self.Pu = torch.empty((q, d), **f32), torch.empty((q, d), **f32)
        self.dPi, self.dPu = torch.empty((q, d), **f32), torch.empty((q, d), **f32)
        self._raw = torch.zeros(6, **f32)  # [bpr, reg_lambda reg, lse_u, pos_u, lse_i, pos_i] as the kernels leave them
        self._scaled = torch.zeros(6, **f32)
        lam = self.ssl_lambda
        self._factors = torch.tensor([1.0, 1.0, lam, -lam, lam, -lam], **f32)
        self._ones = torch.ones(2, **f32)
        self._nce_ws = {}

    def prefetch(self, users, pos, neg):
        """Nothing to prepare ahead: the step's index work is inside its calls."""

    # ---- forward (every row): F, T and the two projections
    @torch.no_grad()
    def forward(self):
        K, U = self.K, self.U
        prev = self.P
        for l in range(1, K + 1):
            last = l == K
            cur = self.E[(l - 1) & 1]
            ops.spmm_ex_raw(self.G, prev, Y=cur, sum_in=self.P if l == 1 else self.S, sum_out=self.F if last else self.S)
            prev = cur
        ops.lincomb_raw(self.T, self.F, 1.0, prev, -1.0)
        ops.lowrank_project_raw(self.svd_v, self.T[U:], out=self.Pi)
        ops.lowrank_project_raw(self.svd_u, self.T[:U], out=self.Pu)
        return self.F

    def _ws(self, B, N):
        key = (B, N)
        ws = self._nce_ws.get(key)
        if ws is None:
            ws = self._nce_ws[key] = ops.svd_nce_workspace(B, N, self.d, self.q, self.device)
        return ws

    # ---- one training step: losses [bpr, reg_lambda reg, ssl_lambda ssl]
    @torch.no_grad()
    def train_step(self, users, pos, neg, loss_out=None):
        K, U, I = self.K, self.U, self.I
        B = int(users.shape[0])
        loss = self.loss if loss_out is None else loss_out
        users, pos, neg = (t if t.dtype == torch.int64 and t.is_contiguous() else t.long().contiguous() for t in (users, pos, neg))
        self.forward()
        self.GF.zero_()
        self.GE.zero_()
        ops.bpr_fwd_bwd_raw(self.F, self.P, users, pos, neg, U, self.reg_lambda, self._ones, self.GF, self.GE, self._raw[0:2])
        up = self._factors[2:4]
        ops.svd_nce_raw(self.F, self.P, 0, U, self.us, self.Pi, users, self.temperature, loss=self._raw[2:4], upstream=up,
                        g_final=self.GF, g_ego=self.GE, dP=self.dPi, ws=self._ws(B, U))
        ops.svd_nce_raw(self.F, self.P, U, I, self.vs, self.Pu, pos, self.temperature, loss=self._raw[4:6], upstream=up,
                        g_final=self.GF, g_ego=self.GE, dP=self.dPu, ws=self._ws(B, I))
        torch.mul(self._raw, self._factors, out=self._scaled)
        loss[0:2].copy_(self._scaled[0:2])
        torch.sum(self._scaled[2:6], dim=0, keepdim=True, out=loss[2:3])
        # P_i = V^T T_i reads the ITEM rows of T and feeds the USER side's view: gT_i = V dP_i, gT_u = U dP_u
        ops.lowrank_expand_raw(self.svd_v, self.dPi, Y=self.GT[U:])
        ops.lowrank_expand_raw(self.svd_u, self.dPu, Y=self.GT[:U])
        ops.lincomb_raw(self.GT, self.GT, 1.0, self.GF, 1.0)  # gF + gT: the addend of every product of the chain
        self.step_count += 1
        h = self.GF
        for k in range(K - 1, 0, -1):
            nxt = self.H[k % len(self.H)]
            ops.spmm_ex_raw(self.G, h, Y=nxt, addend=self.GT)
            h = nxt
        ops.spmm_ex_raw(self.G, h, addend=self.GT, sum_in=self.GE, sum_out=self.GRAD)
        ops.adam_step_raw(self.P, self.GRAD, self.M, self.V, self.lr, self.step_count, self.betas[0], self.betas[1], self.eps)
        return loss
