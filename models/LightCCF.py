"""LightCCF (Zhang et al., SIGIR'25) on MI355X: BPR, the regulariser and the neighbour-aggregation loss — an in-batch
contrastive term whose negatives are the batch's positives AND the batch's users, `a_i.b_j + a_i.a_j` inside one exponential
(reference: models/LightCCF.py).

The encoder is plain matrix factorisation (`encoder = MF`: the embedding tables themselves; no graph is attached) or, for any
other value — as the reference treats every non-MF string — LightGCN (the layer mean of A^k E0, k = 0..GCN_layer).  The new
term is one fused operator (idg_na_nce_f32): one rectangular Gram problem a_i.(a_j + b_j) over 128 x 128 score tiles of the
batch rows as they come, formed twice (row sums, then the gradient weights, which need the finished sums because of the 1e-5
inside the log) and never stored as a [B, B] matrix.  The trainer's fused step adds that call behind BPR inside the LightGCN /
MF training chain.
"""
import torch

import utility.utility_data.data_graph as data_graph
import utility.utility_train.trainer as trainer
from idgrec_amd import ops
from idgrec_amd.modeling import PackedRecommender


class LightCCF(PackedRecommender):
    include_layer0 = True  # LightGCN encoder: E0 takes part in the layer mean (models/LightCCF.py:41-57)
    supports_fused_step = True
    n_fused_losses = 3
    margin = None  # LightCSCF sets one

    def __init__(self, config, dataset, device):
        super(LightCCF, self).__init__(config, dataset, device)
        self.ssl_lambda = float(config['ssl_lambda'])
        self.temperature = float(config['temperature'])
        self.encoder = config['encoder']
        if self.encoder == 'MF':
            self.n_layers = 0
        else:
            self.n_layers = int(config['GCN_layer'])
            self.attach_graph(data_graph.sparse_adjacency_matrix(dataset))

    def engine(self):
        eng = super().engine()
        eng.na = (self.temperature, self.ssl_lambda, None, True)
        return eng

    def _final(self):
        ego = self.ego_panel()
        return ego, (ops.propagate_mean(self.Graph, ego, self.n_layers, include_layer0=True) if self.n_layers > 0 else ego)

    def aggregate(self):
        """(users [U,d], items [I,d]): the encoder's output."""
        return torch.split(self._final()[1], [self.dataset.num_users, self.dataset.num_items])

    def forward(self, user, positive, negative):
        ego, final = self._final()
        U = self.dataset.num_users
        bpr, reg = ops.bpr_loss(final, ego, user, positive, negative, U, self.reg_lambda)
        na = ops.na_nce_loss(final, user, positive, U, self.temperature, None, self.ssl_lambda)
        return [bpr, reg, na]


class Trainer():
    def __init__(self, args, config, dataset, device, logger):
        self.model = LightCCF(config, dataset, device)
        self.args, self.config, self.dataset = args, config, dataset
        self.device, self.logger = device, logger

    def train(self):
        trainer.universal_trainer(self.model, self.args, self.config, self.dataset, self.device, self.logger)
