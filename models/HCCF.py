"""HCCF (Xia et al., SIGIR'22: "Hypergraph Contrastive Collaborative Filtering") on MI355X — reference: models/HCCF.py.

Every layer has a graph branch and a hypergraph branch over the same input X_l (X_0 = the ego panel E0):
    S_l = G X_l                                        ("gnn_embeddings[l]": the library's SpMM operator)
    H_s = dropout(E0_s W_s, p = 1 - keeprate)          per side s (users with user_hyper_emb, items with item_hyper_emb),
    Y_l[s] = H_s (H_s^T X_l[s])                        ("hyper_embeddings[l]": ops.hyper_mix), a fresh mask per layer and side
    X_l+1 = S_l + Y_l,   final = X_0 + .. + X_K        (the SUM, ego layer included)
and BPR on final, the regulariser on the batch's ego rows and both hyperedge matrices, and per layer two in-batch InfoNCE
terms on the RAW batch rows, S_l (detached) against Y_l at the users and at the positives (ops.infonce_pair, dedup off).
At (embedding_size, hyper_size) = (64, 64) ops.hyper_mix runs on the four kernels of csrc/idg_hyper.hip — H is never stored,
the mask is a function of (seed, stream, row, hyperedge) — and the model trains through the fused, autograd-free step of
idgrec_amd/hccf.py; at other widths ops.hyper_mix composes torch operators and the step runs under autograd.

As in the reference, F.dropout has no training= switch: evaluation draws masks too (its aggregate() has no evaluation
branch) — here once per evaluation pass, cached while the weights are frozen.  keeprate = 1.0 (the configuration's) keeps
everything.  The reference's dropedge() is never called and is not ported."""
import torch
from torch import nn

import utility.utility_data.data_graph as data_graph
import utility.utility_function.losses as losses
import utility.utility_train.trainer as trainer
from idgrec_amd import ops
from idgrec_amd.hccf import HccfEngine
from idgrec_amd.modeling import EngineStep, PackedRecommender


class HCCF(EngineStep, PackedRecommender):
    #: trains through a fused chain of library calls (idgrec_amd/hccf.py) at (embedding_size, hyper_size) = (64, 64);
    #: otherwise through the differentiable operators below
    supports_fused_step = True
    n_fused_losses = 3
    include_layer0 = True
    #: None, or a callable returning the [GCN_layer, n, hyper_size] uint8 / bool keep masks of the next forward / fused step /
    #: evaluation pass (tests feed the reference's recorded draws through it)
    mask_source = None

    def __init__(self, config, dataset, device):
        rng = torch.get_rng_state()
        super(HCCF, self).__init__(config, dataset, device)
        self.n_layers = int(config['GCN_layer'])
        self.keeprate = float(config['keeprate'])
        if self.n_layers < 1 or not 0.0 < self.keeprate <= 1.0:
            raise ValueError("HCCF needs GCN_layer >= 1 and 0 < keeprate <= 1 (got GCN_layer = %d, keeprate = %g)"
                             % (self.n_layers, self.keeprate))
        self.ssl_lambda = float(config['ssl_lambda'])
        self.temperature = float(config['temperature'])
        d, h = int(config['embedding_size']), int(config['hyper_size'])
        # The reference constructs its four nn.Embedding first and initialises them afterwards (models/HCCF.py:26-40); the
        # base class has constructed AND initialised the two tables.  Replay the reference's order of draws from the generator
        # state of before, so that a given torch seed gives the reference's initial values.
        torch.set_rng_state(rng)
        for w in (self.user_embedding.weight, self.item_embedding.weight):
            torch.empty(w.shape).normal_()
        self.user_hyper_emb = nn.Embedding(num_embeddings=d, embedding_dim=h)
        self.item_hyper_emb = nn.Embedding(num_embeddings=d, embedding_dim=h)
        for emb in (self.user_embedding, self.item_embedding, self.user_hyper_emb, self.item_hyper_emb):
            nn.init.xavier_uniform_(emb.weight, gain=1.)
        self.attach_graph(data_graph.sparse_adjacency_matrix(dataset))

    # ------------------------------------------------------------------ fused path (trainer protocol)
    def fused_step_available(self):
        st = self._storage
        if st is None or not st.is_cuda:
            return False
        return int(st.shape[1]) == 64 and tuple(self.user_hyper_emb.weight.shape) == (64, 64)

    def hccf_engine(self):
        """The fused engine over the packed embedding panel; the two hyperedge matrices move into ITS flat buffer (the
        nn.Parameters are re-pointed at views of it), so one Adam launch updates both."""
        if not self._is_packed():
            self._pack()
        eng = getattr(self, "_hccf_engine", None)
        if not self._engine_is_current(eng):
            eng = self._hccf_engine = self._adopt_engine(HccfEngine(
                self.Graph, self.dataset.num_users, self.dataset.num_items, self._storage,
                (self.user_hyper_emb.weight.data, self.item_hyper_emb.weight.data), self.n_layers, keep=self.keeprate,
                reg_lambda=self.reg_lambda, ssl_lambda=self.ssl_lambda, temperature=self.temperature))
        return eng

    _fused_engine = hccf_engine

    def _engine_params(self):
        return [self.user_embedding.weight, self.item_embedding.weight, self.user_hyper_emb.weight, self.item_hyper_emb.weight]

    def _step_kwargs(self):
        return dict(masks=self._masks())

    # ------------------------------------------------------------------ differentiable path
    def _masks(self):
        return None if self.mask_source is None else self.mask_source()

    def aggregate(self, masks=None):
        """(final [n, d], [S_l], [Y_l]), as the reference's aggregate(): users first in every panel."""
        U = self.dataset.num_users
        ego = self.ego_panel()
        if masks is None:
            masks = self._masks()
        x, total, gnn, hyper = ego, ego, [], []
        for l in range(self.n_layers):
            s = ops.spmm(self.Graph, x)
            stream = ops._next_noise_stream()  # ONE stream for both sides of a layer: the draws are indexed by the global row
            mu, mi = (None, None) if masks is None else (masks[l, :U], masks[l, U:])
            yu = ops.hyper_mix(ego[:U], self.user_hyper_emb.weight, x[:U], row0=0, keep=self.keeprate, stream=stream, mask=mu)
            yi = ops.hyper_mix(ego[U:], self.item_hyper_emb.weight, x[U:], row0=U, keep=self.keeprate, stream=stream, mask=mi)
            y = torch.cat([yu, yi])
            x = s + y
            total = total + x
            gnn.append(s)
            hyper.append(y)
        return total, gnn, hyper

    def forward(self, user, positive, negative, masks=None):
        U = self.dataset.num_users
        user, positive, negative = user.long(), positive.long(), negative.long()
        final, gnn, hyper = self.aggregate(masks)
        bpr_loss, reg_loss = ops.bpr_loss(final, self.ego_panel(), user, positive, negative, U, self.reg_lambda)
        # get_reg_loss(.., user_hyper_emb.weight, item_hyper_emb.weight): 1/2 ||W||^2 / W.shape[0] each (losses.py:16-21)
        reg_loss = reg_loss + self.reg_lambda * losses.get_reg_loss(self.user_hyper_emb.weight, self.item_hyper_emb.weight)
        ssl_loss = 0.
        for s, y in zip(gnn, hyper):
            # both terms of a layer in one call: the users' rows and the positives' rows, raw ids (duplicates count)
            ssl_loss = ssl_loss + ops.infonce_pair(s.detach(), y, user, positive, U, self.temperature, dedup=False)
        return [bpr_loss, reg_loss, self.ssl_lambda * ssl_loss]

    def _eval_panels(self):
        with torch.no_grad():
            U = self.dataset.num_users
            final = self.aggregate()[0]
            return final[:U].contiguous(), final[U:].contiguous()

    def get_rating_for_test(self, user, masks=None):
        """sigmoid(final_u[user] . final_i^T) (models/HCCF.py:121-127).  masks = None: the panels of this evaluation pass (one
        draw, cached while the weights are frozen); a [GCN_layer, n, hyper_size] panel: final with exactly those masks."""
        if masks is None:
            return super(HCCF, self).get_rating_for_test(user)
        with torch.no_grad():
            U = self.dataset.num_users
            final = self.aggregate(masks)[0]
            return ops.score_dense(final[:U].contiguous(), final[U:].contiguous(), user.long(), apply_sigmoid=True)


class Trainer():
    def __init__(self, args, config, dataset, device, logger):
        self.model = HCCF(config, dataset, device)
        self.args, self.config, self.dataset = args, config, dataset
        self.device, self.logger = device, logger

    def train(self):
        trainer.universal_trainer(self.model, self.args, self.config, self.dataset, self.device, self.logger)
