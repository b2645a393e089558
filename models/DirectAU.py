"""DirectAU (Wang et al., KDD'22) on MI355X: alignment + uniformity of the normalised (user, positive item) rows in
place of a ranking loss; negatives are drawn by the trainer as usual and ignored (reference: models/DirectAU.py).

The encoder is LightGCN (`encoder = LightGCN`: the layer mean of A^k E0, k = 0..GCN_layer) or plain matrix factorisation
(`encoder = MF`: the embedding tables themselves; no graph is built, as in the reference, so the torch RNG stream is
consumed the same way).  The loss triple [align, gamma * uniform, reg_lambda * reg] is one fused operator
(idg_align_uniform_f32): the uniformity term runs over every pair of the batch's rows in 64 x 64 tiles without storing
the B x B matrix.  The trainer's fused step puts that call in place of BPR inside the LightGCN / MF training chain.
"""
import torch

import utility.utility_data.data_graph as data_graph
import utility.utility_train.trainer as trainer
from idgrec_amd import ops
from idgrec_amd.modeling import PackedRecommender


class DirectAU(PackedRecommender):
    include_layer0 = True  # LightGCN encoder: E0 takes part in the layer mean (models/DirectAU.py:41-48)
    supports_fused_step = True
    n_fused_losses = 3

    def __init__(self, config, dataset, device):
        super(DirectAU, self).__init__(config, dataset, device)
        self.gamma = float(config['gamma'])
        self.encoder = config['encoder']
        if self.encoder == 'LightGCN':
            self.n_layers = int(config['GCN_layer'])
            self.attach_graph(data_graph.sparse_adjacency_matrix(dataset))
        elif self.encoder == 'MF':
            self.n_layers = 0
        else:
            raise ValueError("DirectAU: encoder must be LightGCN or MF (got %r)" % self.encoder)

    def engine(self):
        eng = super().engine()
        eng.au = (self.gamma,)
        return eng

    def aggregate(self):
        """(users [U,d], items [I,d]): the encoder's output."""
        ego = self.ego_panel()
        final = ops.propagate_mean(self.Graph, ego, self.n_layers, include_layer0=True) if self.n_layers > 0 else ego
        return torch.split(final, [self.dataset.num_users, self.dataset.num_items])

    def forward(self, user, positive, negative):
        ego = self.ego_panel()
        final = ops.propagate_mean(self.Graph, ego, self.n_layers, include_layer0=True) if self.n_layers > 0 else ego
        align_loss, uniform_loss, reg_loss = ops.align_uniform_loss(final, ego, user, positive, self.dataset.num_users,
                                                                    self.gamma, self.reg_lambda)
        return [align_loss, uniform_loss, reg_loss]


class Trainer():
    def __init__(self, args, config, dataset, device, logger):
        self.model = DirectAU(config, dataset, device)
        self.args, self.config, self.dataset = args, config, dataset
        self.device, self.logger = device, logger

    def train(self):
        trainer.universal_trainer(self.model, self.args, self.config, self.dataset, self.device, self.logger)
