"""LR-GCCF (Chen et al., AAAI'20: "Revisiting Graph based Collaborative Filtering: A Linear Residual Graph Convolutional
Network Approach") on MI355X — reference: models/GCCF.py.

A linear layer per hop, E_l = dropout((G . E_{l-1}) . W_l + b_l) on the self-loop adjacency G = D^-1/2 (A + I) D^-1/2, and
the concatenation [E_0 | E_1 | .. | E_K] as the scored rows: no bilinear term, no activation, no row normalisation.  The
sparse product runs on the library's SpMM operator (symmetric graph: backward reuses the handle; with node_dropout a
re-drawn masked copy of the handle per training forward), the layer on ops.gccf_layer (d = 64: one kernel per direction,
idg_gccf_layer_fwd_f32 / idg_gccf_layer_bwd_f32).  Regularisation covers the positive and negative item rows only.  With
layer_size = [64] * K and node dropout off the model trains through the fused, autograd-free step of idgrec_amd/gccf.py."""
import torch
from torch import nn

import utility.utility_data.data_graph as data_graph
import utility.utility_function.losses as losses
import utility.utility_train.trainer as trainer
from idgrec_amd import ops
from idgrec_amd.gccf import GccfEngine
from idgrec_amd.modeling import EngineStep, PackedRecommender


class GCCF(EngineStep, PackedRecommender):
    #: trains through a fused chain of library calls (idgrec_amd/gccf.py) when d = 64, every layer maps d -> d and node
    #: dropout is off; otherwise through the differentiable operators below
    supports_fused_step = True
    n_fused_losses = 2

    def __init__(self, config, dataset, device):
        super(GCCF, self).__init__(config, dataset, device)
        self.n_layers = int(config['GCN_layer'])
        if self.n_layers < 1:
            raise ValueError("GCCF needs GCN_layer >= 1: its rows are the concatenation of the embedding and K linear layers "
                             "(got GCN_layer = %d)" % self.n_layers)
        widths = [int(config['embedding_size'])] + eval(config['layer_size'])
        self.weight_dict = nn.ParameterDict()
        for layer in range(self.n_layers):  # creation order = the reference's torch RNG order
            for name, shape in (('W_gcn_%d', (widths[layer], widths[layer + 1])), ('b_gcn_%d', (1, widths[layer + 1]))):
                self.weight_dict[name % layer] = nn.Parameter(nn.init.xavier_uniform_(torch.empty(*shape)))
        if eval(config['mess_dropout']):
            self.mess_dropout = eval(config['mess_drop_prob'])
        self.node_dropout = bool(eval(config['node_dropout']))
        if self.node_dropout and 'node_keep_prob' not in config:
            # the reference's aggregate() reads node_keep_prob, which its settings file does not carry (it has node_drop_prob)
            raise ValueError("GCCF with node_dropout = True reads the key node_keep_prob, which the configuration lacks")
        self.node_keep_prob = float(config['node_keep_prob']) if self.node_dropout else 1.0
        self.attach_graph(data_graph.sparse_adjacency_matrix_with_self(dataset))

    # ------------------------------------------------------------------ fused path (trainer protocol)
    def fused_step_available(self):
        st = self._storage
        if st is None or not st.is_cuda or not hasattr(self, "mess_dropout") or self.node_dropout:
            return False
        d = int(st.shape[1])
        return d == 64 and all(tuple(self.weight_dict['W_gcn_%d' % l].shape) == (d, d) for l in range(self.n_layers))

    def gccf_engine(self):
        """The fused engine over the packed embedding panel; the 2K small tensors move into ITS flat buffer (the
        nn.Parameters are re-pointed at views of it), so one Adam launch updates all of them."""
        if not self._is_packed():
            self._pack()
        eng = getattr(self, "_gccf_engine", None)
        if not self._engine_is_current(eng):
            w = self.weight_dict
            small = [(w['W_gcn_%d' % l].data, w['b_gcn_%d' % l].data) for l in range(self.n_layers)]
            eng = self._gccf_engine = self._adopt_engine(GccfEngine(
                self.Graph, self.dataset.num_users, self.dataset.num_items, self._storage, small,
                mess_dropout=self.mess_dropout, reg_lambda=self.reg_lambda))
        return eng

    _fused_engine = gccf_engine

    def _engine_params(self):
        """The two tables, then every layer's (W_gcn, b_gcn): the order of self.parameters() and of the engine."""
        return [self.user_embedding.weight, self.item_embedding.weight] + list(self.weight_dict.values())

    def aggregate(self):
        ego = self.ego_panel()
        layers = [ego]
        # node dropout (models/GCCF.py:49-58, 67-73): ONE re-drawn edge mask per training forward, shared by the layers;
        # on the device it is a masked copy of the handle (same tile schedule; backward multiplies by the transposed mask)
        graph = self.Graph
        if self.node_dropout and self.training:
            graph = self._dropped = self.Graph.dropout_copy(self.node_keep_prob, reuse=getattr(self, "_dropped", None))
        w = self.weight_dict
        for layer in range(self.n_layers):
            # The reference instantiates nn.Dropout inside aggregate() (models/GCCF.py:84): a fresh module is always in
            # training mode, so message dropout is applied during evaluation as well — kept as is
            ego = ops.gccf_layer(ops.spmm(graph, ego), w['W_gcn_%d' % layer], w['b_gcn_%d' % layer], self.mess_dropout[layer])
            layers.append(ego)
        final = torch.cat(layers, dim=1)
        return torch.split(final, [self.dataset.num_users, self.dataset.num_items])

    def forward(self, user, positive, negative):
        all_user, all_item = self.aggregate()
        bpr_loss = losses.get_bpr_loss(all_user[user.long()], all_item[positive.long()], all_item[negative.long()])
        # get_reg_loss(item_embedding(positive), item_embedding(negative)) (models/GCCF.py:100-105; losses.py:16-21):
        # sum_b 1/2 ||W[pos_b]||^2 + 1/2 ||W[neg_b]||^2 over the batch = sum_i count_i * 1/2 ||W_i||^2, which autograd
        # differentiates as one dense product instead of two sort-based embedding backward passes
        W = self.item_embedding.weight
        count = torch.bincount(torch.cat([positive.long(), negative.long()]), minlength=W.shape[0]).to(W.dtype)
        reg_loss = 0.5 * (count * (W * W).sum(dim=1)).sum() / float(len(user))
        return [bpr_loss, self.reg_lambda * reg_loss]

    def _eval_panels(self):
        with torch.no_grad():
            users, items = self.aggregate()
            return users.contiguous(), items.contiguous()


class Trainer():
    def __init__(self, args, config, dataset, device, logger):
        self.model = GCCF(config, dataset, device)
        self.args, self.config, self.dataset = args, config, dataset
        self.device, self.logger = device, logger

    def train(self):
        trainer.universal_trainer(self.model, self.args, self.config, self.dataset, self.device, self.logger)
