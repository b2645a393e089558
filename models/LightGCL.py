"""LightGCL (Cai et al., ICLR'23: "LightGCL: Simple Yet Effective Graph Contrastive Learning for Recommendation") on MI355X —
reference: models/LightGCL.py.

LightGCN propagation SUMMED over the layers 0 .. K (F), BPR on F, the regulariser on the batch's ego rows, and a contrastive
term between F and a rank-q SVD view of it: per side, mean_b log(sum_j exp(<g_b, F_j> / tau) + 1e-8) over the WHOLE table on
raw dot products, minus the clamped positive mean_b clamp(<F_b, g_b> / tau, -5, 5).

The reference propagates with the rectangular D_u^-1/2 R D_i^-1/2 and its transpose; that pair is one product with the
symmetric adjacency the library tiles (data_graph.sparse_adjacency_matrix: its user-row block IS that matrix), so the graph
part is ops.spmm.  The reference's per-layer views g^l = (U S)(V^T E_i^(l-1)), summed, collapse by linearity to
G_u = E_u^0 + (U S) P_i with P_i = V^T T_i, T = F - E^K (and the mirror image for items): two ops.lowrank_project calls, and
ops.svd_nce_loss (idg_svd_nce_f32, csrc/idg_svdnce.hip) forms the batch's view rows itself — neither an [n, d] view panel nor
the [B, N] score matrix is stored.  With a tiled embedding width the model trains through the fused, autograd-free step of
idgrec_amd/lightgcl.py.  The factors come from ONE torch.svd_lowrank at construction, as in the reference (plumbing, not hot
path).  The reference's commented-out sparse_dropout is not here."""
import numpy as np
import torch

import utility.utility_data.data_graph as data_graph
import utility.utility_train.trainer as trainer
from idgrec_amd import ops
from idgrec_amd.lightgcl import LightgclEngine
from idgrec_amd.modeling import EngineStep, PackedRecommender


def svd_factors(R_hat, q, device):
    """(svd_u [U, q], s [q], svd_v [I, q]) float32 on `device`: torch.svd_lowrank(R_hat, q) of the scipy matrix R_hat as a
    coalesced sparse tensor — on the device where torch takes the sparse operand there, on the host otherwise."""
    coo = R_hat.tocoo()
    idx = torch.from_numpy(np.vstack([coo.row, coo.col]).astype(np.int64))
    sp = torch.sparse_coo_tensor(idx, torch.from_numpy(coo.data.astype(np.float32)), coo.shape).coalesce()
    try:
        out = torch.svd_lowrank(sp.to(device), q=q)
    except (RuntimeError, NotImplementedError):
        out = torch.svd_lowrank(sp, q=q)
    return tuple(t.to(device=device, dtype=torch.float32).contiguous() for t in out)


class LightGCL(EngineStep, PackedRecommender):
    #: trains through a fused chain of library calls (idgrec_amd/lightgcl.py) at embedding_size 32 / 64 / 128 / 256;
    #: otherwise through the differentiable operators below
    supports_fused_step = True
    n_fused_losses = 3
    include_layer0 = True
    FUSED_WIDTHS = (32, 64, 128, 256)
    #: None, or (svd_u, s, svd_v) to use in place of torch.svd_lowrank's (tests feed the reference's recorded factors)
    factor_source = None

    def __init__(self, config, dataset, device):
        super(LightGCL, self).__init__(config, dataset, device)
        self.n_layers = int(config['GCN_layer'])
        if self.n_layers < 1:
            raise ValueError("LightGCL needs GCN_layer >= 1: its SVD view is built from the layers below the last "
                             "(got GCN_layer = %d)" % self.n_layers)
        self.ssl_lambda = float(config['ssl_lambda'])
        self.temperature = float(config['temperature'])
        self.svd_q = int(config['svd_q'])
        if not 1 <= self.svd_q <= ops.LOWRANK_MAX_RANK:
            raise ValueError("LightGCL: svd_q = %d (ranks 1 .. %d are built)" % (self.svd_q, ops.LOWRANK_MAX_RANK))
        if not self.temperature > 0:
            raise ValueError("LightGCL: temperature must be positive (got %r)" % (self.temperature,))
        adj = data_graph.sparse_adjacency_matrix(dataset)
        self.attach_graph(adj)
        U = dataset.num_users
        if self.factor_source is None:
            factors = svd_factors(adj[:U, U:], self.svd_q, torch.device(self.device))
        else:
            factors = tuple(torch.as_tensor(t).to(device=torch.device(self.device), dtype=torch.float32).contiguous()
                            for t in self.factor_source)
        self.set_factors(*factors)

    def set_factors(self, svd_u, s, svd_v):
        """Install (svd_u [U, q], s [q], svd_v [I, q]); an engine built on other factors is dropped."""
        U, I = self.dataset.num_users, self.dataset.num_items
        q = int(s.shape[0])
        if tuple(svd_u.shape) != (U, q) or tuple(svd_v.shape) != (I, q):
            raise ValueError("LightGCL: factors %s, %s, %s for %d users and %d items" % (tuple(svd_u.shape), tuple(s.shape),
                                                                                          tuple(svd_v.shape), U, I))
        self.svd_u, self.svd_s, self.svd_v = svd_u, s, svd_v
        self.u_mul_s, self.v_mul_s = (svd_u * s).contiguous(), (svd_v * s).contiguous()
        self._lightgcl_engine = None

    # ------------------------------------------------------------------ fused path (trainer protocol)
    def lightgcl_engine(self):
        """The fused engine over the packed embedding panel."""
        if not self._is_packed():
            self._pack()
        eng = getattr(self, "_lightgcl_engine", None)
        if not self._engine_is_current(eng):
            eng = self._lightgcl_engine = self._adopt_engine(LightgclEngine(
                self.Graph, self.dataset.num_users, self.dataset.num_items, self._storage, self.n_layers, self.svd_u, self.svd_s,
                self.svd_v, reg_lambda=self.reg_lambda, ssl_lambda=self.ssl_lambda, temperature=self.temperature))
        return eng

    _fused_engine = lightgcl_engine

    def _engine_params(self):
        return [self.user_embedding.weight, self.item_embedding.weight]

    # ------------------------------------------------------------------ differentiable path
    def _sum_layers(self):
        """(F [n, d], E^K, ego): the layers 0 .. K summed, the last layer, the ego panel; users first."""
        ego = self.ego_panel()
        x, total = ego, ego
        for _ in range(self.n_layers):
            x = ops.spmm(self.Graph, x)
            total = total + x
        return total, x, ego

    def aggregate(self):
        """(users, items): the summed layers (the reference's first two results; its two view panels are never formed)."""
        total, _, _ = self._sum_layers()
        return torch.split(total, [self.dataset.num_users, self.dataset.num_items])

    def forward(self, user, positive, negative):
        U, I = self.dataset.num_users, self.dataset.num_items
        user, positive, negative = user.long(), positive.long(), negative.long()
        F, last, ego = self._sum_layers()
        T = F - last
        P_i = ops.lowrank_project(self.svd_v, T[U:])
        P_u = ops.lowrank_project(self.svd_u, T[:U])
        bpr_loss, reg_loss = ops.bpr_loss(F, ego, user, positive, negative, U, self.reg_lambda)
        lse_u, pos_u = ops.svd_nce_loss(F, ego, 0, U, self.u_mul_s, P_i, user, self.temperature)
        lse_i, pos_i = ops.svd_nce_loss(F, ego, U, I, self.v_mul_s, P_u, positive, self.temperature)
        ssl_loss = self.ssl_lambda * (-(pos_u + pos_i) + (lse_u + lse_i))
        return [bpr_loss, reg_loss, ssl_loss]

    def _eval_panels(self):
        with torch.no_grad():
            users, items = self.aggregate()
            return users.contiguous(), items.contiguous()


class Trainer():
    def __init__(self, args, config, dataset, device, logger):
        self.model = LightGCL(config, dataset, device)
        self.args, self.config, self.dataset = args, config, dataset
        self.device, self.logger = device, logger

    def train(self):
        trainer.universal_trainer(self.model, self.args, self.config, self.dataset, self.device, self.logger)
