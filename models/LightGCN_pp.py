"""LightGCN++ (Lee et al., RecSys'24: "Revisiting LightGCN: Unexpected Inflexibility, Inconsistency, and A Remedy Towards
Improved Recommendation") on MI355X — reference: models/LightGCN_pp.py.

LightGCN's loss, trainer and evaluator over a different encoder:

    adjacency   A' = D^-alpha A D^-beta with alpha != beta, so A' != A'^T (data_graph.sparse_adjacency_matrix_asymmetric);
                the handle carries its transposed twin and the backward products run on Graph.T.
    layers      X_k = A' rownorm(X_(k-1)), rownorm(x) = x / (||x||_2 + 1e-12) per row, X_0 = E0 — ops.rows_normalize_raw /
                idg_rows_normalize_f32 in front of every product.
    output      gamma E0 + (1 - gamma) mean(X_1 .. X_K): E0 is weighted on its own and not averaged in.

forward() is ops.propagate_normalized + ops.bpr_loss under autograd.  The fused step is one fixed chain of library calls: K x
(rows_normalize_raw + spmm_ex_raw with the running sum, and on the last product the division by K, in its epilogue),
lincomb_raw for the output, bpr_fused_raw, K x (Graph.T.spmm_raw + rows_normalize_bwd_raw, which folds in the output's
direct gradient share and, at layer 0, the regulariser's gradient), and the dense adam_step_raw.  The products run over the
whole panel.
"""
import torch

import utility.utility_data.data_graph as data_graph
import utility.utility_train.trainer as trainer
from idgrec_amd import ops
from idgrec_amd.modeling import PackedRecommender


class LightGCN_pp(PackedRecommender):
    supports_fused_step = True  # loss == [bpr, reg]
    n_fused_losses = 2
    _buf = None

    def __init__(self, config, dataset, device):
        super(LightGCN_pp, self).__init__(config, dataset, device)
        self.gamma = float(config['gamma'])
        self.alpha = float(config['alpha'])
        self.beta = float(config['beta'])
        self.n_layers = int(config['GCN_layer'])
        if self.n_layers < 1:
            raise ValueError("LightGCN_pp needs GCN_layer >= 1: its output averages the propagated layers X_1 .. X_K "
                             "(got GCN_layer = %d)" % self.n_layers)
        self.attach_graph(data_graph.sparse_adjacency_matrix_asymmetric(dataset, self.alpha, self.beta))

    def attach_graph(self, sp_mat):
        """Upload the adjacency with its transposed twin: A' != A'^T."""
        from utility.utility_function import tools

        dev = torch.device(self.device)
        if dev.type != "cuda":
            raise RuntimeError("%s needs an MI355X: device is %s and idgrec_amd has no CPU path "
                               "(torch.cuda.is_available() = %s)." % (type(self).__name__, dev, torch.cuda.is_available()))
        self.Graph = tools.convert_sp_mat_to_graph(sp_mat, dev, symmetric=False)
        return self.Graph

    # ------------------------------------------------------------------ the reference's surface
    def aggregate(self):
        """(users [U,d], items [I,d]) = gamma E0 + (1 - gamma) mean_k X_k (models/LightGCN_pp.py:75-96)."""
        final = ops.propagate_normalized(self.Graph, self.ego_panel(), self.n_layers, self.gamma)
        return torch.split(final, [self.dataset.num_users, self.dataset.num_items])

    def forward(self, user, positive, negative):
        ego = self.ego_panel()
        final = ops.propagate_normalized(self.Graph, ego, self.n_layers, self.gamma)
        bpr_loss, reg_loss = ops.bpr_loss(final, ego, user, positive, negative, self.dataset.num_users, self.reg_lambda)
        return [bpr_loss, reg_loss]

    def _eval_panels(self):
        with torch.no_grad():
            if not self._is_packed():
                self._pack()
            fin = ops.propagate_normalized(self.Graph, self._storage, self.n_layers, self.gamma)
        U = self.dataset.num_users
        return fin[:U], fin[U:]

    # ------------------------------------------------------------------ fused step
    def _step_buffers(self):
        """Allocated once per storage: the normalised inputs N_0 .. N_(K-1) with their norms, the running sum / layer mean,
        the output and its gradient, the regulariser's gradient, the two panels the backward chain alternates between."""
        st = self._storage
        if self._buf is None or self._buf["key"] != (st.data_ptr(), st.device):
            K = self.n_layers
            new = lambda: torch.empty_like(st)  # noqa: E731
            self._buf = dict(key=(st.data_ptr(), st.device), N=[new() for _ in range(K)],
                             norms=[torch.empty(st.shape[0], dtype=torch.float32, device=st.device) for _ in range(K)],
                             S=new(), final=new(), g_final=new(), g_reg=new(), chain=[new(), new()], grad=None)
        return self._buf

    def fused_loss_and_grad(self, users, pos, neg, loss_out=None):
        """Losses [bpr, reg_lambda * reg] (device tensor) and d(sum) / d(weights) in the two parameters' .grad, as one fixed
        chain of library calls."""
        if not self._is_packed():
            self._pack()
        st = self._storage
        U, K, gamma = self.dataset.num_users, self.n_layers, self.gamma
        users, pos, neg = (t.long().contiguous() for t in (users, pos, neg))
        buf = self._step_buffers()
        self._eval_cache = None
        if loss_out is None:
            loss_out = torch.empty(self.n_fused_losses, dtype=torch.float32, device=st.device)
        N, norms, S, g_final, g_reg = buf["N"], buf["norms"], buf["S"], buf["g_final"], buf["g_reg"]
        # X_k = A' N_(k-1) lands in N[k] and is normalised there; the last product only feeds the sum, divided by K
        for k in range(1, K + 1):
            last = k == K
            ops.rows_normalize_raw(st if k == 1 else N[k - 1], Y=N[k - 1], norms=norms[k - 1])
            ops.spmm_ex_raw(self.Graph, N[k - 1], Y=None if last else N[k], sum_in=None if k == 1 else S, sum_out=S,
                            div=float(K) if last else 1.0)
        ops.lincomb_raw(buf["final"], st, gamma, S, 1.0 - gamma)
        g_final.zero_()
        g_reg.zero_()
        ops.bpr_fused_raw(buf["final"], st, users, pos, neg, U, self.reg_lambda, g_final, g_reg, loss=loss_out[0:2])
        # H_K = c g; H_(k-1) = a g + J_(k-1)(A'^T H_k), a = c above layer 0 and gamma at it, where the regulariser's gradient joins
        c = (1.0 - gamma) / K
        H, T = buf["chain"]
        ops.lincomb_raw(H, g_final, c)
        for k in range(K, 0, -1):
            self.Graph.T.spmm_raw(H, out=T)
            ops.rows_normalize_bwd_raw(T, N[k - 1], norms[k - 1], G=g_final, a=c if k > 1 else gamma,
                                       add2=g_reg if k == 1 else None, out=T)
            H, T = T, H
        buf["grad"] = H
        self.user_embedding.weight.grad = H[:U]
        self.item_embedding.weight.grad = H[U:]
        return loss_out

    def fused_train_step(self, users, pos, neg, loss_out, optimizer):
        """fused_loss_and_grad + the dense Adam step of the packed panel, in the state of `optimizer` as _packed_adam hands it
        over.  False — nothing done — when it does not."""
        adam = self._packed_adam(optimizer)
        if adam is None:
            return False
        group, st_u, st_i, (m, v) = adam
        self.fused_loss_and_grad(users, pos, neg, loss_out)
        step = int(st_u["step"]) + 1
        b1, b2 = group["betas"]
        ops.adam_step_raw(self._storage, self._buf["grad"], m, v, group["lr"], step, b1, b2, group["eps"])
        st_u["step"] = st_i["step"] = step
        if not getattr(self, "keep_fused_grad", False):
            self.user_embedding.weight.grad = self.item_embedding.weight.grad = None
        return True

    def prefetch_batch(self, users, pos, neg):
        """Nothing to prepare ahead: the step's index work is inside its calls."""


class Trainer():
    def __init__(self, args, config, dataset, device, logger):
        self.model = LightGCN_pp(config, dataset, device)
        self.args, self.config, self.dataset = args, config, dataset
        self.device, self.logger = device, logger

    def train(self):
        trainer.universal_trainer(self.model, self.args, self.config, self.dataset, self.device, self.logger)
