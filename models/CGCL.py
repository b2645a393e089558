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

The fused step is LayerChainRecommender's (idgrec_amd/modeling.py: every layer kept, the fused BPR on the layer mean, the
backward chain, a dense Adam step); CGCL states that layers 0, 1 and 2 carry a gradient panel and issues the four calls.
"""
import utility.utility_data.data_graph as data_graph
import utility.utility_train.trainer as trainer
from idgrec_amd import ops
from idgrec_amd.modeling import LayerChainRecommender


class CGCL(LayerChainRecommender):
    include_layer0 = True  # E0 takes part in the layer mean (models/CGCL.py:44-60)
    n_fused_losses = 5
    ssl_layers = (0, 1, 2)  # center, candidate, context: layers above 2 carry no contrastive term
    ssl_parts = (4, 2)  # one row per call of _terms(), one entry per query block

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

    # ------------------------------------------------------------------ the reference's surface
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

    # ------------------------------------------------------------------ fused step: the hook of LayerChainRecommender
    def _ssl_raw(self, E, G, users, pos, parts, loss_out):
        item_rows = pos + self.dataset.num_users
        for c, (tl, row0, N, blocks, user_side) in enumerate(self._terms()):
            q_ids = item_rows if user_side else users
            ops.table_nce_raw(E[tl], row0, N, [E[ql] for ql, _, _ in blocks], [q_ids] * len(blocks),
                              users if user_side else pos, [w for _, w, _ in blocks], self.temperature,
                              loss=parts[c, :len(blocks)], g_table=G[tl], g_queries=[G[ql] for ql, _, _ in blocks])
        loss_out[2:4] = parts[0] + parts[1]
        loss_out[4] = parts[2, 0] + parts[3, 0]


class Trainer():
    def __init__(self, args, config, dataset, device, logger):
        self.model = CGCL(config, dataset, device)
        self.args, self.config, self.dataset = args, config, dataset
        self.device, self.logger = device, logger

    def train(self):
        trainer.universal_trainer(self.model, self.args, self.config, self.dataset, self.device, self.logger)
