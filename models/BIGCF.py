"""BIGCF (Zhang et al., SIGIR'24: "Exploring the Individuality and Collectivity of Intents behind Interactions for Graph
Collaborative Filtering") on MI355X — reference: models/BIGCF.py.

LightGCN propagation without the ego layer, summed (X = G E + .. + G^K E), then the intent layer on every row — one intent
matrix for the user rows, one for the item rows:
    T = softmax(X W) W^T  (the "collective intent" rows),   F = X + T * Z,  Z ~ N(0, 1) redrawn every forward
and BPR on F, the regulariser on the batch's ego rows and both intent matrices, and five in-batch InfoNCE terms on the RAW
batch rows: F[users] and F[pos] each against themselves, F[users] against F[pos], T[users] and T[pos] each against themselves.
The propagation runs on the library's SpMM operator, the intent layer on ops.intent_mix ((64, 128): one kernel per direction,
idg_intent_fwd_f32 / idg_intent_bwd_f32, Z generated on the device from (seed, stream, row, feature) and never stored); in
forward() the InfoNCE terms are evaluated in float64 on the gathered batch rows (see there).  With embedding_size = 64 and
intent_size = 128 the model trains through the fused, autograd-free step of idgrec_amd/bigcf.py.  Evaluation draws noise
too, as the reference does (its aggregate() has no evaluation branch): once per evaluation pass.  int_temperature is read
and unused, as in the reference."""
import torch
from torch import nn

import utility.utility_data.data_graph as data_graph
import utility.utility_function.losses as losses
import utility.utility_train.trainer as trainer
from idgrec_amd import ops
from idgrec_amd.bigcf import BigcfEngine
from idgrec_amd.modeling import EngineStep, PackedRecommender


class BIGCF(EngineStep, PackedRecommender):
    #: trains through a fused chain of library calls (idgrec_amd/bigcf.py) at (embedding_size, intent_size) = (64, 128);
    #: otherwise through the differentiable operators below
    supports_fused_step = True
    n_fused_losses = 3
    include_layer0 = False
    #: None, or a callable returning the [n, d] noise panel of the next forward / fused step / evaluation pass (tests feed
    #: the reference's recorded draws through it)
    noise_source = None

    def __init__(self, config, dataset, device):
        rng = torch.get_rng_state()
        super(BIGCF, self).__init__(config, dataset, device)
        self.n_layers = int(config['GCN_layer'])
        if self.n_layers < 1:
            raise ValueError("BIGCF needs GCN_layer >= 1: its rows are the sum of the propagated layers, the ego layer left out "
                             "(got GCN_layer = %d)" % self.n_layers)
        self.ssl_lambda = float(config['ssl_lambda'])
        self.ssl_temperature = float(config['ssl_temperature'])
        self.int_temperature = float(config['int_temperature'])  # read and unused, as in the reference
        d, k = int(config['embedding_size']), int(config['intent_size'])
        # The reference constructs its four nn.Embedding first and initialises them afterwards (models/BIGCF.py:24-38); the
        # base class has constructed AND initialised the two tables.  Replay the reference's order of draws from the generator
        # state of before, so that a given torch seed gives the reference's initial values.
        torch.set_rng_state(rng)
        for w in (self.user_embedding.weight, self.item_embedding.weight):
            torch.empty(w.shape).normal_()
        self.user_intent = nn.Embedding(num_embeddings=d, embedding_dim=k)
        self.item_intent = nn.Embedding(num_embeddings=d, embedding_dim=k)
        for emb in (self.user_embedding, self.item_embedding, self.user_intent, self.item_intent):
            nn.init.xavier_uniform_(emb.weight, gain=1.)
        self.attach_graph(data_graph.sparse_adjacency_matrix(dataset))

    # ------------------------------------------------------------------ fused path (trainer protocol)
    def fused_step_available(self):
        st = self._storage
        if st is None or not st.is_cuda:
            return False
        return int(st.shape[1]) == 64 and tuple(self.user_intent.weight.shape) == (64, 128)

    def bigcf_engine(self):
        """The fused engine over the packed embedding panel; the two intent matrices move into ITS flat buffer (the
        nn.Parameters are re-pointed at views of it), so one Adam launch updates both."""
        if not self._is_packed():
            self._pack()
        eng = getattr(self, "_bigcf_engine", None)
        if not self._engine_is_current(eng):
            eng = self._bigcf_engine = self._adopt_engine(BigcfEngine(
                self.Graph, self.dataset.num_users, self.dataset.num_items, self._storage,
                (self.user_intent.weight.data, self.item_intent.weight.data), self.n_layers, reg_lambda=self.reg_lambda,
                ssl_lambda=self.ssl_lambda, temperature=self.ssl_temperature))
        return eng

    _fused_engine = bigcf_engine

    def _engine_params(self):
        return [self.user_embedding.weight, self.item_embedding.weight, self.user_intent.weight, self.item_intent.weight]

    def _step_kwargs(self):
        return dict(noise=self._noise())

    # ------------------------------------------------------------------ differentiable path
    def _noise(self):
        return None if self.noise_source is None else self.noise_source()

    def _mix(self, noise=None):
        """(F [n, d], T [n, d], ego): the intent layer on the propagated panel, users first."""
        U = self.dataset.num_users
        ego = self.ego_panel()
        x, total = ego, None
        for _ in range(self.n_layers):
            x = ops.spmm(self.Graph, x)
            total = x if total is None else total + x
        if noise is None:
            noise = self._noise()
        stream = ops._next_noise_stream()  # ONE stream for both blocks: the draws are indexed by the global row
        Fu, Tu = ops.intent_mix(total[:U], self.user_intent.weight, row0=0, stream=stream, noise=None if noise is None else noise[:U])
        Fi, Ti = ops.intent_mix(total[U:], self.item_intent.weight, row0=U, stream=stream, noise=None if noise is None else noise[U:])
        return torch.cat([Fu, Fi]), torch.cat([Tu, Ti]), ego

    def aggregate(self, noise=None):
        """(users, items, users' intent rows, items' intent rows), as the reference's aggregate()."""
        U, I = self.dataset.num_users, self.dataset.num_items
        F, T, _ = self._mix(noise)
        return torch.split(F, [U, I]) + torch.split(T, [U, I])

    def forward(self, user, positive, negative, noise=None):
        U = self.dataset.num_users
        user, positive, negative = user.long(), positive.long(), negative.long()
        F, T, ego = self._mix(noise)
        bpr_loss, reg_loss = ops.bpr_loss(F, ego, user, positive, negative, U, self.reg_lambda)
        # get_reg_loss(.., user_intent.weight, item_intent.weight): 1/2 ||W||^2 / W.shape[0] each (losses.py:16-21)
        reg_loss = reg_loss + self.reg_lambda * losses.get_reg_loss(self.user_intent.weight, self.item_intent.weight)
        # The five in-batch InfoNCE terms (models/BIGCF.py:92-102) on the gathered [B, d] rows, evaluated in FLOAT64.  Measured
        # on the reference's fixture: a float32 evaluation of these terms' gradients (this library's kernels and torch's
        # alike: 3e-6 .. 8e-6 of their largest entry at temperature 0.2) is where nine tenths of the distance of this path's
        # table gradients from a float64 evaluation of the whole model comes from; every other stage together adds 2e-10 next
        # to a largest entry of 2e-2.  Five [B, B] matrices in float64 cost this path 2.3 ms of its 4.1 ms step at B = 2048
        # (scripts/bigcf_step.py); it is not the training hot path: the fused step (idgrec_amd/bigcf.py, 1.19 ms) runs the
        # terms on idg_infonce_pair_f32 — one panel as both views and both gradients — and idg_infonce_cross_ex_f32.
        t = self.ssl_temperature
        fu, fp = F[user].double(), F[U + positive].double()
        tu, tp = T[user].double(), T[U + positive].double()
        ssl = losses.get_InfoNCE_loss(fu, fu, t) + losses.get_InfoNCE_loss(fp, fp, t) + losses.get_InfoNCE_loss(fu, fp, t) \
            + losses.get_InfoNCE_loss(tu, tu, t) + losses.get_InfoNCE_loss(tp, tp, t)
        ssl = ssl.to(F.dtype)
        return [bpr_loss, reg_loss, self.ssl_lambda * ssl]

    def _eval_panels(self):
        with torch.no_grad():
            users, items, _, _ = self.aggregate()
            return users.contiguous(), items.contiguous()

    def get_rating_for_test(self, user, noise=None):
        """sigmoid(F_u[user] . F_i^T) (models/BIGCF.py:108-114).  noise = None: the panels of this evaluation pass (one draw,
        cached while the weights are frozen); a [n, d] panel: F with exactly that noise."""
        if noise is None:
            return super(BIGCF, self).get_rating_for_test(user)
        with torch.no_grad():
            users, items, _, _ = self.aggregate(noise)
            return ops.score_dense(users.contiguous(), items.contiguous(), user.long(), apply_sigmoid=True)


class Trainer():
    def __init__(self, args, config, dataset, device, logger):
        self.model = BIGCF(config, dataset, device)
        self.args, self.config, self.dataset = args, config, dataset
        self.device, self.logger = device, logger

    def train(self):
        trainer.universal_trainer(self.model, self.args, self.config, self.dataset, self.device, self.logger)
