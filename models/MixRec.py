"""MixRec (Zhang et al., WWW'25: "MixRec: Individual and Collective Mixing Empowers Data Augmentation for Recommender
Systems") on MI355X — reference: models/MixRec.py.

LightGCN propagation without the ego layer, summed (X = G E + .. + G^K E), BPR on X weighted by the step's item_beta, the
regulariser on the batch's ego rows, and contrastive terms whose operands exist only inside the batch: rows mixed pairwise
with a Beta weight along a random permutation ("individual" mixing), one Dirichlet-weighted mix of all the batch's rows
("collective" mixing) as an extra negative, and the positives kept OUT of the negative sets.  The propagation runs on the
library's SpMM operator, BPR and the regulariser on ops.bpr_loss, all contrastive terms on ONE fused operator, ops.mix_nce
(idg_mix_nce_f32, csrc/idg_mixnce.hip: two Gram problems and one rectangular one, no [B, B] matrix stored).  With a tiled
embedding width the model trains through the fused, autograd-free step of idgrec_amd/mixrec.py.  The reference's
mix_aggregate() is dead code and is not here."""
import torch

import utility.utility_data.data_graph as data_graph
import utility.utility_train.trainer as trainer
from idgrec_amd import ops
from idgrec_amd.mixrec import MixrecEngine, draw_mix
from idgrec_amd.modeling import EngineStep, PackedRecommender


class MixRec(EngineStep, PackedRecommender):
    #: trains through a fused chain of library calls (idgrec_amd/mixrec.py) at embedding_size 32 / 64 / 128 / 256;
    #: otherwise through the differentiable operators below
    supports_fused_step = True
    n_fused_losses = 4
    include_layer0 = False
    FUSED_WIDTHS = (32, 64, 128, 256)
    #: None, or a callable returning the five host draws of the next forward / fused step — (user_beta, item_beta, nu [B],
    #: user_perm [B], item_perm [B]) — in place of mixrec.draw_mix (tests feed the reference's recorded draws through it)
    mix_source = None

    def __init__(self, config, dataset, device):
        super(MixRec, self).__init__(config, dataset, device)
        self.n_layers = int(config['GCN_layer'])
        if self.n_layers < 1:
            raise ValueError("MixRec needs GCN_layer >= 1: its rows are the sum of the propagated layers, the ego layer left out "
                             "(got GCN_layer = %d)" % self.n_layers)
        self.ssl_lambda = float(config['ssl_lambda'])
        self.temperature = float(config['temperature'])
        self.alpha, self.beta, self.gamma = float(config['alpha']), float(config['beta']), float(config['gamma'])
        self.attach_graph(data_graph.sparse_adjacency_matrix(dataset))

    # ------------------------------------------------------------------ fused path (trainer protocol)
    def mixrec_engine(self):
        """The fused engine over the packed embedding panel."""
        if not self._is_packed():
            self._pack()
        eng = getattr(self, "_mixrec_engine", None)
        if not self._engine_is_current(eng):
            eng = self._mixrec_engine = self._adopt_engine(MixrecEngine(
                self.Graph, self.dataset.num_users, self.dataset.num_items, self._storage, self.n_layers,
                reg_lambda=self.reg_lambda, ssl_lambda=self.ssl_lambda, temperature=self.temperature, alpha=self.alpha,
                beta=self.beta, gamma=self.gamma))
        return eng

    _fused_engine = mixrec_engine

    def _engine_params(self):
        return [self.user_embedding.weight, self.item_embedding.weight]

    def _step_kwargs(self):
        return dict(draws=None if self.mix_source is None else self.mix_source())

    # ------------------------------------------------------------------ differentiable path
    def _draws(self, B):
        return draw_mix(B, self.alpha, self.beta, self.gamma) if self.mix_source is None else self.mix_source()

    def _sum_layers(self):
        """(X [n, d], ego): the propagated layers summed, users first."""
        ego = self.ego_panel()
        x, total = ego, None
        for _ in range(self.n_layers):
            x = ops.spmm(self.Graph, x)
            total = x if total is None else total + x
        return total, ego

    def aggregate(self):
        """(users, items), as the reference's aggregate()."""
        total, _ = self._sum_layers()
        return torch.split(total, [self.dataset.num_users, self.dataset.num_items])

    def forward(self, user, positive, negative):
        U = self.dataset.num_users
        user, positive, negative = user.long(), positive.long(), negative.long()
        X, ego = self._sum_layers()
        user_beta, item_beta, nu, user_perm, item_perm = self._draws(int(user.shape[0]))
        dev = X.device
        bpr_loss, reg_loss = ops.bpr_loss(X, ego, user, positive, negative, U, self.reg_lambda)
        mix_loss, ssl_loss = ops.mix_nce(X, U, user, positive, negative, torch.as_tensor(user_perm).to(dev),
                                         torch.as_tensor(item_perm).to(dev), torch.as_tensor(nu, dtype=torch.float32).to(dev),
                                         user_beta, item_beta, self.temperature, self.ssl_lambda)
        return [float(item_beta) * bpr_loss, mix_loss, reg_loss, ssl_loss]

    def _eval_panels(self):
        with torch.no_grad():
            users, items = self.aggregate()
            return users.contiguous(), items.contiguous()


class Trainer():
    def __init__(self, args, config, dataset, device, logger):
        self.model = MixRec(config, dataset, device)
        self.args, self.config, self.dataset = args, config, dataset
        self.device, self.logger = device, logger

    def train(self):
        trainer.universal_trainer(self.model, self.args, self.config, self.dataset, self.device, self.logger)
