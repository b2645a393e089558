"""GCMC (van den Berg et al., "Graph Convolutional Matrix Completion", in the form of the NGCF code base) on MI355X —
reference: models/GCMC.py.

Two chained transforms per hop on the plain bipartite adjacency G = D^-1/2 A D^-1/2 (no self loops: LightGCN's graph):
    side = G . ego;  M = leaky_relu(side . W_gcn + b_gcn, 0.2) . W_mlp + b_mlp;  ego = dropout(M);  N = normalize(ego)
and the concatenation [E_0 | N_1 | .. | N_K] as the scored rows; the un-normalised ego feeds the next hop.  The sparse product
runs on the library's SpMM operator (symmetric graph: backward reuses the handle), the layer on ops.gcmc_layer (both
matrices [64, 64]: one kernel per direction, idg_gcmc_layer_fwd_f32 / idg_gcmc_layer_bwd_f32).  Regularisation covers the
user, positive and negative ego rows.  With embedding_size = 64 and the first GCN_layer entries of layer_size equal to 64 the
model trains through the fused, autograd-free step of idgrec_amd/gcmc.py.  The reference never calls its node_dropout method
and its settings file has no such key: there is no node dropout here."""
import torch
from torch import nn

import utility.utility_data.data_graph as data_graph
import utility.utility_function.losses as losses
import utility.utility_train.trainer as trainer
from idgrec_amd import ops
from idgrec_amd.gcmc import GcmcEngine
from idgrec_amd.modeling import EngineStep, PackedRecommender

NAMES = ('W_gcn_%d', 'b_gcn_%d', 'W_mlp_%d', 'b_mlp_%d')


class GCMC(EngineStep, PackedRecommender):
    #: trains through a fused chain of library calls (idgrec_amd/gcmc.py) when d = 64, every layer maps d -> d and message
    #: dropout is on; otherwise through the differentiable operators below
    supports_fused_step = True
    n_fused_losses = 2

    def __init__(self, config, dataset, device):
        super(GCMC, self).__init__(config, dataset, device)
        self.n_layers = int(config['GCN_layer'])
        if self.n_layers < 1:
            raise ValueError("GCMC needs GCN_layer >= 1: its rows are the concatenation of the embedding and K normalised "
                             "layers (got GCN_layer = %d)" % self.n_layers)
        widths = [int(config['embedding_size'])] + eval(config['layer_size'])
        if len(widths) <= self.n_layers:
            raise ValueError("GCMC: layer_size %s names fewer than GCN_layer = %d widths" % (config['layer_size'], self.n_layers))
        self.weight_dict = nn.ParameterDict()
        for layer in range(self.n_layers):  # creation order = the reference's torch RNG order
            d_in, d_out = widths[layer], widths[layer + 1]
            # W_mlp multiplies the d_out-wide activation.  The reference shapes it [d_in, d_out], which multiplies only
            # where d_in = d_out — there the two shapes (and the random numbers drawn for them) are the same
            for name, shape in zip(NAMES, ((d_in, d_out), (1, d_out), (d_out, d_out), (1, d_out))):
                self.weight_dict[name % layer] = nn.Parameter(nn.init.xavier_uniform_(torch.empty(*shape)))
        if eval(config['mess_dropout']):
            self.mess_dropout = eval(config['mess_drop_prob'])
        self.attach_graph(data_graph.sparse_adjacency_matrix(dataset))

    # ------------------------------------------------------------------ fused path (trainer protocol)
    def fused_step_available(self):
        st = self._storage
        if st is None or not st.is_cuda or not hasattr(self, "mess_dropout"):
            return False
        d = int(st.shape[1])
        return d == 64 and all(tuple(self.weight_dict[nm % l].shape) == (d, d) for l in range(self.n_layers)
                               for nm in ('W_gcn_%d', 'W_mlp_%d'))

    def gcmc_engine(self):
        """The fused engine over the packed embedding panel; the 4K small tensors move into ITS flat buffer (the
        nn.Parameters are re-pointed at views of it), so one Adam launch updates all of them."""
        if not self._is_packed():
            self._pack()
        eng = getattr(self, "_gcmc_engine", None)
        if not self._engine_is_current(eng):
            w = self.weight_dict
            small = [tuple(w[nm % l].data for nm in NAMES) for l in range(self.n_layers)]
            eng = self._gcmc_engine = self._adopt_engine(GcmcEngine(
                self.Graph, self.dataset.num_users, self.dataset.num_items, self._storage, small,
                mess_dropout=self.mess_dropout, reg_lambda=self.reg_lambda))
        return eng

    _fused_engine = gcmc_engine

    def _engine_params(self):
        """The two tables, then every layer's (W_gcn, b_gcn, W_mlp, b_mlp): the order of self.parameters() and of the engine."""
        return [self.user_embedding.weight, self.item_embedding.weight] + list(self.weight_dict.values())

    def aggregate(self):
        ego = self.ego_panel()
        layers = [ego]
        w = self.weight_dict
        for layer in range(self.n_layers):
            # The reference instantiates nn.Dropout inside aggregate() (models/GCMC.py:86): a fresh module is always in
            # training mode, so message dropout is applied during evaluation as well — kept as is
            ego, norm = ops.gcmc_layer(ops.spmm(self.Graph, ego), *(w[nm % layer] for nm in NAMES), self.mess_dropout[layer])
            layers.append(norm)
        final = torch.cat(layers, dim=1)
        return torch.split(final, [self.dataset.num_users, self.dataset.num_items])

    def forward(self, user, positive, negative):
        all_user, all_item = self.aggregate()
        bpr_loss = losses.get_bpr_loss(all_user[user.long()], all_item[positive.long()], all_item[negative.long()])
        # get_reg_loss(user_embedding(user), item_embedding(positive), item_embedding(negative)) (models/GCMC.py:105-112;
        # losses.py:16-21): sum_b 1/2 |row_b|^2 over the three lists = sum_r count_r * 1/2 |row_r|^2 per table, which
        # autograd differentiates as one dense product instead of three sort-based embedding backward passes
        reg_loss = 0.0
        for W, ids in ((self.user_embedding.weight, user.long()), (self.item_embedding.weight, torch.cat([positive.long(), negative.long()]))):
            count = torch.bincount(ids, minlength=W.shape[0]).to(W.dtype)
            reg_loss = reg_loss + 0.5 * (count * (W * W).sum(dim=1)).sum()
        return [bpr_loss, self.reg_lambda * reg_loss / float(len(user))]

    def _eval_panels(self):
        with torch.no_grad():
            users, items = self.aggregate()
            return users.contiguous(), items.contiguous()


class Trainer():
    def __init__(self, args, config, dataset, device, logger):
        self.model = GCMC(config, dataset, device)
        self.args, self.config, self.dataset = args, config, dataset
        self.device, self.logger = device, logger

    def train(self):
        trainer.universal_trainer(self.model, self.args, self.config, self.dataset, self.device, self.logger)
