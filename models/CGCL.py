"""CGCL (He et al., SIGIR'23: candidate-aware graph contrastive learning) on MI355X — reference: models/CGCL.py.

LightGCN + BPR, plus three contrastive terms between the layers' outputs E0 (center), E1 (candidate) and E2 (context).
Each term has a user side and an item side, and each side scores the batch's normalised rows against a WHOLE normalised
user or item table: -sum_b log(exp(q_b . t_pos / tau) / sum_j exp(q_b . t_j / tau) + 1e-7).  The six sides are four calls
of one fused operator (ops.table_nce_loss / idg_table_nce_f32: the [B, N] score matrix is never stored), the two sides
that share a table going into one call:

    table      query blocks (weight)                                                               positive
    E0 users   E2 items[pos]  (layer, ssl_lambda_alpha alpha);  E1 items[pos]  (candidate, ssl_lambda_beta beta)      user
    E0 items   E2 users[user] (layer, .. (1 - alpha));          E1 users[user] (candidate, .. (1 - beta))             pos
    E1 users   E2 items[pos]  (struct, ssl_lambda_gamma gamma)                                                        user
    E1 items   E2 users[user] (struct, .. (1 - gamma))                                                                pos

The fused step runs the same chain without autograd: K products keeping every layer, the fused BPR on the layer mean, the
four calls adding into per-layer gradient panels, the backward chain g_k = A g_(k+1) + g_mean / (K + 1) + g_ssl_k, and a
dense Adam step (the table gradients reach every row).
"""
import torch

import utility.utility_data.data_graph as data_graph
import utility.utility_train.trainer as trainer
from idgrec_amd import ops
from idgrec_amd.modeling import PackedRecommender


class CGCL(PackedRecommender):
    include_layer0 = True  # E0 takes part in the layer mean (models/CGCL.py:44-60)
    supports_fused_step = True
    n_fused_losses = 5

    def __init__(self, config, dataset, device):
        super(CGCL, self).__init__(config, dataset, device)
        self.ssl_lambda_alpha = float(config['ssl_lambda_alpha'])
        self.ssl_lambda_beta = float(config['ssl_lambda_beta'])
        self.ssl_lambda_gamma = float(config['ssl_lambda_gamma'])
        self.alpha = float(config['alpha'])
        self.beta = float(config['beta'])
        self.gamma = float(config['gamma'])
        self.temperature = float(config['temperature'])
        self.n_layers = int(config['GCN_layer'])
        if self.n_layers < 2:
            raise ValueError("CGCL needs GCN_layer >= 2: its contrastive terms compare the outputs of layers 0, 1 and 2 "
                             "(got GCN_layer = %d)" % self.n_layers)
        self.attach_graph(data_graph.sparse_adjacency_matrix(dataset))
        self._buf = None

    # ------------------------------------------------------------------ the reference's surface
    def _layers(self):
        """([E0, E1, .., EK], their mean [n, d])."""
        layers = [self.ego_panel()]
        for _ in range(self.n_layers):
            layers.append(ops.spmm(self.Graph, layers[-1]))
        return layers, torch.stack(layers, dim=1).mean(dim=1)

    def aggregate(self):
        """(users [U,d], items [I,d], [E0, E1, .., EK]): the layer mean and every layer's output (models/CGCL.py:44-60)."""
        layers, final = self._layers()
        users, items = torch.split(final, [self.dataset.num_users, self.dataset.num_items])
        return users, items, layers

    def _terms(self):
        """The four calls: (table layer, row0, N, [(query layer, weight, slot of the loss triple)], the table is the users')."""
        U, I = self.dataset.num_users, self.dataset.num_items
        la, lb, lg = self.ssl_lambda_alpha, self.ssl_lambda_beta, self.ssl_lambda_gamma
        a, b, g = self.alpha, self.beta, self.gamma
        return [(0, 0, U, [(2, la * a, 0), (1, lb * b, 1)], True),
                (0, U, I, [(2, la * (1 - a), 0), (1, lb * (1 - b), 1)], False),
                (1, 0, U, [(2, lg * g, 2)], True),
                (1, U, I, [(2, lg * (1 - g), 2)], False)]

    def forward(self, user, positive, negative):
        """[bpr, reg_lambda * reg, layer, candidate, struct] (models/CGCL.py:62-93)."""
        U = self.dataset.num_users
        user, positive = user.long(), positive.long()
        layers, final = self._layers()
        bpr_loss, reg_loss = ops.bpr_loss(final, layers[0], user, positive, negative, U, self.reg_lambda)
        item_rows = positive + U
        ssl = [0.0, 0.0, 0.0]
        for tl, row0, N, blocks, user_side in self._terms():
            # a user table is scored by the positives' rows of the later layer, an item table by the users' rows
            q_ids = item_rows if user_side else user
            out = ops.table_nce_loss(layers[tl], row0, N, [layers[ql] for ql, _, _ in blocks], [q_ids] * len(blocks),
                                     user if user_side else positive, [w for _, w, _ in blocks], self.temperature)
            for (_, _, slot), term in zip(blocks, out):
                ssl[slot] = ssl[slot] + term
        return [bpr_loss, reg_loss] + ssl

    # ------------------------------------------------------------------ fused, autograd-free step
    def _step_buffers(self):
        st = self._storage
        if self._buf is None or self._buf["key"] != (st.data_ptr(), st.device):
            K = self.n_layers
            new = lambda: torch.empty_like(st)  # noqa: E731
            self._buf = dict(key=(st.data_ptr(), st.device), E=[None] + [new() for _ in range(K)], S=new(), final=new(),
                             g_final=new(), G=[new() for _ in range(3)], chain=[new(), new()], grad=None,
                             parts=torch.empty((4, 2), dtype=torch.float32, device=st.device))
        return self._buf

    def fused_loss_and_grad(self, users, pos, neg, loss_out=None):
        """The five losses (device tensor) and d(sum) / d(weights) in the two parameters' .grad, as one fixed chain of library
        calls."""
        if not self._is_packed():
            self._pack()
        st = self._storage
        U, K = self.dataset.num_users, self.n_layers
        users, pos, neg = (t.long().contiguous() for t in (users, pos, neg))
        buf = self._step_buffers()
        self._eval_cache = None
        if loss_out is None:
            loss_out = torch.empty(5, dtype=torch.float32, device=st.device)
        E, G = buf["E"], buf["G"]
        E[0] = st
        # layers 1..K and their mean: the running sum rides in the product's epilogue
        for k in range(1, K + 1):
            last = k == K
            ops.spmm_ex_raw(self.Graph, E[k - 1], Y=E[k], sum_in=E[0] if k == 1 else buf["S"],
                            sum_out=buf["final"] if last else buf["S"], div=float(K + 1) if last else 1.0)
        for t in (buf["g_final"], G[0], G[1], G[2]):
            t.zero_()
        # BPR on the mean; the regulariser's gradient lands with layer 0's
        ops.bpr_fused_raw(buf["final"], st, users, pos, neg, U, self.reg_lambda, buf["g_final"], G[0], loss=loss_out[0:2])
        item_rows = pos + U
        parts = buf["parts"].zero_()
        for c, (tl, row0, N, blocks, user_side) in enumerate(self._terms()):
            q_ids = item_rows if user_side else users
            ops.table_nce_raw(E[tl], row0, N, [E[ql] for ql, _, _ in blocks], [q_ids] * len(blocks),
                              users if user_side else pos, [w for _, w, _ in blocks], self.temperature,
                              loss=parts[c, :len(blocks)], g_table=G[tl], g_queries=[G[ql] for ql, _, _ in blocks])
        loss_out[2:4] = parts[0] + parts[1]
        loss_out[4] = parts[2, 0] + parts[3, 0]
        # g_k = A g_(k+1) + g_final / (K + 1) + g_ssl_k, from the last layer down (layers above 2 carry no contrastive term)
        share = 1.0 / (K + 1)
        cur = buf["chain"][K % 2]
        if K >= 3:
            ops.lincomb_raw(cur, buf["g_final"], share)
        else:
            ops.lincomb_raw(cur, G[2], 1.0, buf["g_final"], share)
        for k in range(K - 1, -1, -1):
            if k <= 2:
                add = G[k]
                ops.lincomb_raw(add, G[k], 1.0, buf["g_final"], share)
            else:
                add = buf["S"]
                ops.lincomb_raw(add, buf["g_final"], share)
            nxt = buf["chain"][k % 2]
            self.Graph.spmm_raw(cur, addend=add, out=nxt)
            cur = nxt
        buf["grad"] = cur
        self.user_embedding.weight.grad = cur[:U]
        self.item_embedding.weight.grad = cur[U:]
        return loss_out

    def fused_train_step(self, users, pos, neg, loss_out, optimizer):
        """fused_loss_and_grad + the dense Adam step of the packed panel, in the state of `optimizer` (an ops.Adam over exactly
        the two tables; its step / exp_avg / exp_avg_sq stay the single source of truth, the moments re-homed once into
        packed [n, d] panels that the state entries view, as in PackedRecommender).  False — nothing done — otherwise."""
        uw, iw = self.user_embedding.weight, self.item_embedding.weight
        if not isinstance(optimizer, ops.Adam) or len(optimizer.param_groups) != 1:
            return False
        group = optimizer.param_groups[0]
        if len(group["params"]) != 2 or group["params"][0] is not uw or group["params"][1] is not iw:
            return False
        if not self._is_packed():
            self._pack()
        U = self.dataset.num_users
        st_u, st_i = optimizer.state[uw], optimizer.state[iw]
        packed = getattr(self, "_packed_moments", None)
        if (packed is None or packed[0].device != self._storage.device or not st_u or not st_i
                or st_u["exp_avg"].data_ptr() != packed[0].data_ptr() or st_i["exp_avg_sq"].data_ptr() != packed[1][U:].data_ptr()):
            m, v = torch.zeros_like(self._storage), torch.zeros_like(self._storage)
            for st, sl in ((st_u, slice(0, U)), (st_i, slice(U, None))):
                if st:  # the optimizer has already stepped the other way: keep what it accumulated
                    m[sl].copy_(st["exp_avg"])
                    v[sl].copy_(st["exp_avg_sq"])
                st.setdefault("step", 0)
                st["exp_avg"], st["exp_avg_sq"] = m[sl], v[sl]
            packed = self._packed_moments = (m, v)
        if st_u["step"] != st_i["step"]:
            return False
        self.fused_loss_and_grad(users, pos, neg, loss_out)
        step = int(st_u["step"]) + 1
        b1, b2 = group["betas"]
        ops.adam_step_raw(self._storage, self._buf["grad"], packed[0], packed[1], group["lr"], step, b1, b2, group["eps"])
        st_u["step"] = st_i["step"] = step
        if not getattr(self, "keep_fused_grad", False):
            uw.grad = iw.grad = None
        return True

    def prefetch_batch(self, users, pos, neg):
        """Nothing to prepare ahead: the step's index work is inside its calls."""


class Trainer():
    def __init__(self, args, config, dataset, device, logger):
        self.model = CGCL(config, dataset, device)
        self.args, self.config, self.dataset = args, config, dataset
        self.device, self.logger = device, logger

    def train(self):
        trainer.universal_trainer(self.model, self.args, self.config, self.dataset, self.device, self.logger)
