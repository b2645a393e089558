"""IMP-GCN (Liu et al., "Interest-aware Message-Passing GCN for Recommendation", WWW'21) on MI355X — reference:
models/IMPGCN.py.

Every user is assigned to the group(s) whose score is the row's maximum,
    scores = dropout(fc_group(dropout(leaky_relu(fc(E0 + A . E0)))))        (both dropouts p = 0.4, on in training only)
— several groups on a tie, which dropout makes common — and every item to all groups; each group g then propagates on its own
sub-graph A_g = D_g A D_g (values masked, not re-normalised) for GCN_layer - 1 hops from the shared embedding panel, the
groups are summed per hop (hop 0: `group` copies of the panel, the reference's stack-and-sum) and the hops averaged.  The
membership is a comparison: no gradient reaches fc / fc_group, which keep their initial values for ever, as in the reference.

The assignment runs in ONE kernel (ops.group_assign_raw), and one walk of the adjacency serves all groups of a hop
(ops.grouped_propagate -> idg_grouped_spmm_f32; the reference: `group` torch.sparse.mm calls per hop over freshly built
sparse tensors).  With embedding_size = 64 and 1 <= group <= 8 the model trains through the fused, autograd-free step of
idgrec_amd/impgcn.py; other widths compose existing operators."""
import torch
import torch.nn.functional as F
from torch import nn

import utility.utility_data.data_graph as data_graph
import utility.utility_function.losses as losses
import utility.utility_train.trainer as trainer
from idgrec_amd import ops
from idgrec_amd.impgcn import ImpgcnEngine
from idgrec_amd.modeling import EngineStep, PackedRecommender


class IMPGCN(EngineStep, PackedRecommender):
    #: trains through a fused chain of library calls (idgrec_amd/impgcn.py) when d = 64 and 1 <= group <= 8; otherwise
    #: through the differentiable operators below
    supports_fused_step = True
    n_fused_losses = 2

    def __init__(self, config, dataset, device):
        super(IMPGCN, self).__init__(config, dataset, device)
        self.n_layers = int(config['GCN_layer'])
        self.num_groups = int(config['group'])
        if self.n_layers < 1:
            raise ValueError("IMPGCN needs GCN_layer >= 1: its rows are the mean of GCN_layer group sums, the first of them "
                             "`group` copies of the embedding (got GCN_layer = %d)" % self.n_layers)
        if self.num_groups < 1:
            raise ValueError("IMPGCN needs group >= 1 (got group = %d)" % self.num_groups)
        d = int(config['embedding_size'])
        # creation order = the reference's torch RNG order: the two tables (PackedRecommender), then fc, then fc_group
        self.fc = nn.Linear(d, d)
        self.fc_group = nn.Linear(d, self.num_groups)
        self.drop_prob = ops.IMPGCN_DROP
        self._adjacency = data_graph.sparse_adjacency_matrix(dataset)
        self._csr = None
        self.attach_graph(self._adjacency)

    def group_csr(self):
        """The plain device CSR of the adjacency (ops.GroupCsr) next to the ops.Graph handle: made on first use."""
        if self._csr is None or self._csr.graph is not self.Graph:
            self._csr = ops.GroupCsr.from_scipy(self._adjacency, self._storage.device, graph=self.Graph)
        return self._csr

    # ------------------------------------------------------------------ fused path (trainer protocol)
    def fused_step_available(self):
        st = self._storage
        if st is None or not st.is_cuda:
            return False
        return int(st.shape[1]) == 64 and 1 <= self.num_groups <= ops.GROUP_MAX

    def impgcn_engine(self):
        """The fused engine over the packed embedding panel; the four small tensors move into ITS flat buffer (the
        nn.Parameters are re-pointed at views of it)."""
        if not self._is_packed():
            self._pack()
        eng = getattr(self, "_impgcn_engine", None)
        if not self._engine_is_current(eng):
            small = (self.fc.weight.data, self.fc.bias.data, self.fc_group.weight.data, self.fc_group.bias.data)
            eng = self._impgcn_engine = self._adopt_engine(ImpgcnEngine(
                self.Graph, self.group_csr(), self.dataset.num_users, self.dataset.num_items, self._storage, small, self.n_layers,
                p=self.drop_prob, reg_lambda=self.reg_lambda))
        return eng

    _fused_engine = impgcn_engine

    def _engine_params(self):
        """The two tables, then fc.weight, fc.bias, fc_group.weight, fc_group.bias: the order of self.parameters() and of the
        engine."""
        return [self.user_embedding.weight, self.item_embedding.weight, self.fc.weight, self.fc.bias, self.fc_group.weight,
                self.fc_group.bias]

    def fused_loss_and_grad(self, users, pos, neg, loss_out=None):
        """The trainer's fallback when the optimizer is not ours.  The four small tensors take no gradient; they are given a
        ZERO one here, so that an Adam that steps after this call advances all six step counters together (the hand-off to
        the fused step needs them to agree) — a zero gradient leaves the tensor bit-unchanged and its moments zero."""
        out = super().fused_loss_and_grad(users, pos, neg, loss_out)
        for prm in self._engine_params()[2:]:
            if prm.grad is None:
                prm.grad = torch.zeros_like(prm)
        return out

    # ------------------------------------------------------------------ the model
    def membership(self, ego, training):
        """One byte per node: the bitmask of its groups (models/IMPGCN.py:55-64).  No gradient."""
        with torch.no_grad():
            ego = ego.detach()
            side = ops.spmm(self.Graph, ego)
            p = self.drop_prob if training else 0.0
            U, G = self.dataset.num_users, self.num_groups
            if ego.shape[1] == 64 and G <= ops.GROUP_MAX:
                (seed, s_fc), (_, s_grp) = (ops._next_noise_stream(), ops._next_noise_stream()) if p > 0 else ((0, 0), (0, 0))
                return ops.group_assign_raw(ego, side, self.fc.weight, self.fc.bias, self.fc_group.weight, self.fc_group.bias, U, p,
                                            seed, s_fc, s_grp)
            if G > ops.GROUP_MAX:
                raise ValueError("IMPGCN: group = %d above %d (a membership is one byte)" % (G, ops.GROUP_MAX))
            temp = F.dropout(F.leaky_relu(self.fc(ego + side), ops.IMPGCN_SLOPE), p, training)
            scores = F.dropout(self.fc_group(temp), p, training)
            hot = torch.eq(scores, scores.max(dim=1, keepdim=True)[0])
            member = (hot.to(torch.int32) << torch.arange(G, device=ego.device, dtype=torch.int32)).sum(dim=1)
            member[U:] = (1 << G) - 1
            return member.to(torch.uint8)

    def aggregate(self, training=None):
        training = self.training if training is None else training
        ego = self.ego_panel()
        member = self.membership(ego, training)
        G, L = self.num_groups, self.n_layers
        final = float(G) * ego
        if L > 1:
            final = final + ops.grouped_propagate(self.group_csr(), ego, member, L - 1, G, summed=True)
        final = final / float(L)
        return torch.split(final, [self.dataset.num_users, self.dataset.num_items])

    def forward(self, user, positive, negative):
        all_user, all_item = self.aggregate()
        bpr_loss = losses.get_bpr_loss(all_user[user.long()], all_item[positive.long()], all_item[negative.long()])
        # get_reg_loss(user_embedding(user), item_embedding(positive), item_embedding(negative)) (models/IMPGCN.py:97-104): as
        # in models/GCMC.py, sum_r count_r * 1/2 |row_r|^2 per table — one dense product under autograd
        reg_loss = 0.0
        for W, ids in ((self.user_embedding.weight, user.long()), (self.item_embedding.weight, torch.cat([positive.long(), negative.long()]))):
            count = torch.bincount(ids, minlength=W.shape[0]).to(W.dtype)
            reg_loss = reg_loss + 0.5 * (count * (W * W).sum(dim=1)).sum()
        return [bpr_loss, self.reg_lambda * reg_loss / float(len(user))]

    def _eval_panels(self):
        """The evaluation panels: both dropouts off (get_rating_for_test under .eval())."""
        U = self.dataset.num_users
        with torch.no_grad():
            if self.fused_step_available():
                fin = self.impgcn_engine().forward(training=False).clone()
                return fin[:U], fin[U:]
            users, items = self.aggregate(training=False)
            return users.contiguous(), items.contiguous()


class Trainer():
    def __init__(self, args, config, dataset, device, logger):
        self.model = IMPGCN(config, dataset, device)
        self.args, self.config, self.dataset = args, config, dataset
        self.device, self.logger = device, logger

    def train(self):
        trainer.universal_trainer(self.model, self.args, self.config, self.dataset, self.device, self.logger)
