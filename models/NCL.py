"""NCL (Lin et al., WWW'22: neighbourhood-enriched contrastive learning) on MI355X — reference: models/NCL.py.

LightGCN + BPR, plus two contrastive terms on the ego table E0:

    structure   the batch's rows of layer 2 * cl_layer against the WHOLE normalised E0 table of their side, the row's own E0
                row the positive (ssl_layer_loss, models/NCL.py:129-142): ops.table_nce_loss / idg_table_nce_f32, a user
                call (weight ssl_lambda) and an item call (weight ssl_lambda * alpha).
    prototype   in-batch InfoNCE between E0[batch] and the centroid of each row's k-means cluster (models/NCL.py:114-123):
                ops.infonce_pair / idg_infonce_pair_f32 with the raw batch ids, its second view a constant [n, d] panel that
                holds every node's centroid.

The centroids come from the E-step: from epoch `proto_warmup` on (the reference's hard-coded 20) both tables are clustered
at the top of every epoch.  The reference copies them to the host for faiss.Kmeans; here ops.kmeans / idg_kmeans_f32 runs
Lloyd's iterations on the device, on the packed panel in place (DESIGN.md §4 lists the deviations from faiss).

The fused step is LayerChainRecommender's (idgrec_amd/modeling.py: every layer kept, the fused BPR on the layer mean, the
backward chain, a dense Adam step); NCL states that layers 0 and 2 * cl_layer carry a gradient panel and issues the two
full-table calls and, after the warm-up, the prototype call.
"""
import torch

import utility.utility_data.data_graph as data_graph
import utility.utility_train.trainer as trainer
from idgrec_amd import ops
from idgrec_amd.modeling import LayerChainRecommender


class NCL(LayerChainRecommender):
    include_layer0 = True  # E0 takes part in the layer mean (models/NCL.py:48-64)
    n_fused_losses = 4  # [bpr, reg, ssl, proto]; the prototype column is 0 before the warm-up ends
    ssl_parts = (4,)  # structure users, structure items, the prototype call's pair

    def __init__(self, config, dataset, device):
        super(NCL, self).__init__(config, dataset, device)
        self.ssl_lambda = float(config['ssl_lambda'])
        self.proto_lambda = float(config['proto_lambda'])
        self.k = int(config['k'])
        self.alpha = float(config['alpha'])
        self.temperature = float(config['temperature'])
        self.cl_layer = int(config['cl_layer'])
        self.ssl_layers = (0, 2 * self.cl_layer)  # only E0 and the structural term's layer carry a contrastive term
        self.batch_size = int(config['batch_size'])
        self.proto_warmup = int(config.get('proto_warmup', 20))  # models/NCL.py:110,177: `epoch < 20`
        self.kmeans_niter = int(config.get('kmeans_niter', 25))  # faiss.Kmeans' default niter
        self.kmeans_seed = int(config.get('kmeans_seed', 1234))  # faiss.Kmeans' default seed
        self.n_layers = int(config['GCN_layer'])
        if self.cl_layer < 1 or self.n_layers < 2 * self.cl_layer:
            raise ValueError("NCL needs GCN_layer >= 2 * cl_layer >= 2: its structural term reads the output of layer 2 * cl_layer "
                             "(got GCN_layer = %d, cl_layer = %d)" % (self.n_layers, self.cl_layer))
        if self.k < 1 or self.k > min(dataset.num_users, dataset.num_items):
            raise ValueError("NCL: k = %d clusters for tables of %d users and %d items" % (self.k, dataset.num_users,
                                                                                         dataset.num_items))
        self.attach_graph(data_graph.sparse_adjacency_matrix(dataset))
        self.epoch = 0
        self.user_centroids = self.user_2cluster = self.item_centroids = self.item_2cluster = None
        self._proto = None

    # ------------------------------------------------------------------ the reference's surface
    def E_step(self):
        """k-means of the user rows and of the item rows of the packed ego panel, on the device (models/NCL.py:66-81)."""
        if not self._is_packed():
            self._pack()
        U = self.dataset.num_users
        with torch.no_grad():
            st = self._storage
            self.user_centroids, a_u, _ = ops.kmeans(st[:U], self.k, self.kmeans_niter, self.kmeans_seed)
            self.item_centroids, a_i, _ = ops.kmeans(st[U:], self.k, self.kmeans_niter, self.kmeans_seed)
            self.user_2cluster, self.item_2cluster = a_u.long(), a_i.long()
        self._proto = None

    def begin_epoch(self, epoch):
        """The trainer's call at the top of every epoch (models/NCL.py:177-178)."""
        self.epoch = int(epoch)
        if self.epoch >= self.proto_warmup:
            self.E_step()

    def _proto_panel(self):
        """[n, d], row r = the centroid of node r (users first): the constant second view of the prototype term, rebuilt when
        the clusters change."""
        parts = (self.user_centroids, self.user_2cluster, self.item_centroids, self.item_2cluster)
        if any(t is None for t in parts):
            raise RuntimeError("NCL: the prototype term needs clusters: call E_step() (begin_epoch does from epoch %d on)"
                               % self.proto_warmup)
        key = tuple((t.data_ptr(), t._version) for t in parts)
        if self._proto is None or self._proto[0] != key:
            U = self.dataset.num_users
            st = self._storage
            P = torch.empty_like(st)
            for rows, cent, of in ((P[:U], parts[0], parts[1]), (P[U:], parts[2], parts[3])):
                cent = cent.detach().to(device=st.device, dtype=torch.float32).contiguous()
                ops.rows_gather_raw(rows, cent, of.to(st.device).long().contiguous())
            self._proto = (key, P)
        return self._proto[1]

    def forward(self, user, positive, negative, epoch=None):
        """[bpr, reg_lambda * reg, ssl] before the warm-up ends, then [bpr, reg_lambda * reg, ssl, proto]
        (models/NCL.py:83-127)."""
        epoch = self.epoch if epoch is None else int(epoch)
        U, I = self.dataset.num_users, self.dataset.num_items
        user, positive = user.long(), positive.long()
        layers, final = self._layers()
        bpr_loss, reg_loss = ops.bpr_loss(final, layers[0], user, positive, negative, U, self.reg_lambda)
        E0, EL = layers[0], layers[2 * self.cl_layer]
        ssl_u, = ops.table_nce_loss(E0, 0, U, [EL], [user], user, [self.ssl_lambda], self.temperature)
        ssl_i, = ops.table_nce_loss(E0, U, I, [EL], [positive + U], positive, [self.ssl_lambda * self.alpha], self.temperature)
        loss_list = [bpr_loss, reg_loss, ssl_u + ssl_i]
        if epoch < self.proto_warmup:
            return loss_list
        pair = ops.infonce_pair(E0, self._proto_panel(), user, positive, U, self.temperature, dedup=False)
        loss_list.append(self.proto_lambda * self.batch_size * pair)
        return loss_list

    # ------------------------------------------------------------------ fused step: the hook of LayerChainRecommender
    def _ssl_raw(self, E, G, users, pos, parts, loss_out):
        """The prototype entry is 0 before the warm-up ends."""
        U, I, L = self.dataset.num_users, self.dataset.num_items, 2 * self.cl_layer
        G0, GL = G[0], G[L]
        ops.table_nce_raw(E[0], 0, U, [E[L]], [users], users, [self.ssl_lambda], self.temperature, loss=parts[0:1],
                          g_table=G0, g_queries=[GL])
        ops.table_nce_raw(E[0], U, I, [E[L]], [pos + U], pos, [self.ssl_lambda * self.alpha], self.temperature,
                          loss=parts[1:2], g_table=G0, g_queries=[GL])
        loss_out[2] = parts[0] + parts[1]
        if self.epoch >= self.proto_warmup:
            scale = self.proto_lambda * self.batch_size
            # the centroid panel carries no gradient: g2 = None (idg_infonce_pair_f32's final kernel skips a NULL panel)
            ops.infonce_pair_raw(E[0], self._proto_panel(), users, pos, U, self.temperature, g1=G0, g2=None, loss=parts[2:4],
                                 dedup=False, grad_scale=scale, accumulate=True)
            loss_out[3] = (parts[2] + parts[3]) * scale
        else:
            loss_out[3] = 0.0


class Trainer():
    def __init__(self, args, config, dataset, device, logger):
        self.model = NCL(config, dataset, device)
        self.args, self.config, self.dataset = args, config, dataset
        self.device, self.logger = device, logger

    def train(self):
        trainer.universal_trainer(self.model, self.args, self.config, self.dataset, self.device, self.logger)
