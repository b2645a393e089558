"""SCCF (Wu et al., KDD'24) on MI355X: the in-batch second-order contrastive pair [-up, down] over the normalised (user,
positive item) rows in place of a ranking loss; negatives are drawn by the trainer as usual and ignored, and the list
has no regulariser (reference: models/SCCF.py).

The encoder is plain matrix factorisation (`encoder = MF`, the default: the embedding tables themselves; no graph is
attached) or, for any other value — as the reference treats every non-MF string — LightGCN (the layer mean of A^k E0,
k = 0..GCN_layer).  The loss pair is one fused operator (idg_sccf_loss_f32): one rectangular pass over 128 x 128 score tiles
of the batch rows as they come, the two distinct-id counts read off the batch's sorted scatter plan — no torch.unique and no
[Nu, Ni] matrix.  The trainer's fused step puts that call in place of BPR inside the LightGCN / MF training chain.
"""
import torch

import utility.utility_data.data_graph as data_graph
import utility.utility_train.trainer as trainer
from idgrec_amd import ops
from idgrec_amd.modeling import PackedRecommender


class SCCF(PackedRecommender):
    include_layer0 = True  # LightGCN encoder: E0 takes part in the layer mean (models/SCCF.py:40-52)
    supports_fused_step = True
    n_fused_losses = 2

    def __init__(self, config, dataset, device):
        super(SCCF, self).__init__(config, dataset, device)
        self.temperature = float(config['temperature'])
        self.encoder = config['encoder']
        if self.encoder == 'MF':
            self.n_layers = 0
        else:
            self.n_layers = int(config['GCN_layer'])
            self.attach_graph(data_graph.sparse_adjacency_matrix(dataset))

    def engine(self):
        eng = super().engine()
        eng.sccf = (self.temperature,)
        return eng

    def aggregate(self):
        """(users [U,d], items [I,d]): the encoder's output."""
        ego = self.ego_panel()
        final = ops.propagate_mean(self.Graph, ego, self.n_layers, include_layer0=True) if self.n_layers > 0 else ego
        return torch.split(final, [self.dataset.num_users, self.dataset.num_items])

    def forward(self, user, positive, negative):
        ego = self.ego_panel()
        final = ops.propagate_mean(self.Graph, ego, self.n_layers, include_layer0=True) if self.n_layers > 0 else ego
        neg_up, down = ops.sccf_loss(final, user, positive, self.dataset.num_users, self.temperature)
        return [neg_up, down]


class Trainer():
    def __init__(self, args, config, dataset, device, logger):
        self.model = SCCF(config, dataset, device)
        self.args, self.config, self.dataset = args, config, dataset
        self.device, self.logger = device, logger

    def train(self):
        trainer.universal_trainer(self.model, self.args, self.config, self.dataset, self.device, self.logger)
