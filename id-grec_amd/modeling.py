"""Shared machinery of the model plugins in models/*.py.

The reference's models each own two nn.Embedding tables and call torch.cat on them in every
forward (models/LightGCN.py:38).  `PackedRecommender` keeps the same two nn.Embedding
modules (same construction order, hence the same initial weights for a given torch seed) but
backs them with ONE contiguous [num_users + num_items, d] buffer, so the propagation kernels
read the ego panel in place.  It also provides the fused, autograd-free training step and the
fused top-K evaluation that the trainer / evaluator use when a model offers them.
"""
import torch
from torch import nn

from . import ops
from .engine import PropagationEngine


def adam_group_over(optimizer, params):
    """The single param group of `optimizer` when it is an idgrec_amd.ops.Adam over exactly `params` (the same tensors in
    the same order): the gate of every fused_train_step.  None otherwise."""
    if not isinstance(optimizer, ops.Adam) or len(optimizer.param_groups) != 1:
        return None
    group = optimizer.param_groups[0]
    if len(group["params"]) != len(params) or any(a is not b for a, b in zip(group["params"], params)):
        return None
    return group


def adopt_adam_state(optimizer, homes):
    """Make the Adam moments of `optimizer` live where a fused step updates them.  homes: [(parameter, exp_avg home,
    exp_avg_sq home), ...].  A state entry that is empty, or whose exp_avg is not already the home, is re-homed: what the
    optimizer has accumulated is copied in, and the entry then IS the home — the optimizer's state stays the single source of
    truth, whichever way the next step is taken.  Returns the parameters' common step count, or None (the re-homing done all
    the same) when their counters disagree."""
    steps = set()
    for prm, m, v in homes:
        st = optimizer.state[prm]
        if not st or st["exp_avg"].data_ptr() != m.data_ptr():
            if st:  # the optimizer has already stepped the other way: keep what it accumulated
                m.copy_(st["exp_avg"])
                v.copy_(st["exp_avg_sq"])
            st.setdefault("step", 0)
            st["exp_avg"], st["exp_avg_sq"] = m, v
        steps.add(int(st["step"]))
    return steps.pop() if len(steps) == 1 else None


class EngineStep:
    """The trainer protocol (fused_train_step, fused_loss_and_grad, prefetch_batch) of a model whose fused step is an engine
    of its own (NGCF, GCCF, BIGCF: a PanelEngine; EGCF: EgcfEngine / EgcfAltEngine) — a mixin, listed before the nn.Module
    base.  The model supplies fused_step_available() and three things:
        _fused_engine()   its engine getter; after (re)building an engine it calls _adopt_engine(eng)
        _engine_params()  its parameters in the order of the engine's param_views() / moment_homes()
        _step_kwargs()    further keyword arguments of the engine's train_step (default: none)"""
    _fused_params = None  # _engine_params(), listed once
    _fused_homes = None   # [(parameter, exp_avg home, exp_avg_sq home)] in the current engine

    def _fused_engine(self):
        raise NotImplementedError

    def _engine_params(self):
        raise NotImplementedError

    def _step_kwargs(self):
        return {}

    def _step_params(self):
        if self._fused_params is None:
            self._fused_params = self._engine_params()
        return self._fused_params

    def _engine_is_current(self, eng):
        """Whether the parameters still live in `eng`'s storage: not before the first engine, nor after .to() or a re-pack
        has re-created the tensors (the first and the last parameter tell)."""
        if eng is None:
            return False
        params, views = self._step_params(), eng.param_views()
        return params[0].data_ptr() == views[0].data_ptr() and params[-1].data_ptr() == views[-1].data_ptr()

    def _adopt_engine(self, eng):
        """After `eng` was (re)built: the parameters now live in ITS storage — re-point every nn.Parameter at the engine's
        view — and pair them, once, with the homes of their Adam moments."""
        params = self._step_params()
        for prm, view in zip(params, eng.param_views()):
            prm.data = view
        self._fused_homes = [(prm, m, v) for prm, (m, v) in zip(params, eng.moment_homes())]
        return eng

    def _engine_adam(self, optimizer):
        """The hand-off of a fused step to `optimizer`: (param group, common step count), or None — nothing stepped — unless
        it is an idgrec_amd.ops.Adam over exactly _engine_params(), the fused step is available, and the step counters
        agree.  The moments are re-homed into the engine's buffers (adopt_adam_state)."""
        group = adam_group_over(optimizer, self._step_params())
        if group is None or not self.fused_step_available():
            return None
        self._fused_engine()
        step = adopt_adam_state(optimizer, self._fused_homes)
        return None if step is None else (group, step)

    def fused_train_step(self, users, pos, neg, loss_out, optimizer):
        """forward + backward + every Adam update as ONE chain of kernels, in the state of `optimizer` as _engine_adam hands
        it over; False (nothing done) when it does not.  Its state stays the single source of truth."""
        adam = self._engine_adam(optimizer)
        if adam is None:
            return False
        group, step = adam
        eng = self._fused_engine()
        eng.lr, eng.betas, eng.eps = float(group["lr"]), tuple(group["betas"]), float(group["eps"])
        eng.step_count = step
        self._eval_cache = None
        eng.train_step(users, pos, neg, loss_out, **self._step_kwargs())
        for prm in self._fused_params:
            optimizer.state[prm]["step"] = eng.step_count
        return True

    def fused_loss_and_grad(self, users, pos, neg, loss_out=None):
        """The trainer's fallback when the optimizer is not ours: the differentiable operators under autograd."""
        self._eval_cache = None
        ll = self.forward(users, pos, neg)
        self.zero_grad()
        sum(ll).backward()
        out = torch.stack([x.detach() for x in ll])
        if loss_out is not None:
            loss_out.copy_(out)
        return out

    def prefetch_batch(self, users, pos, neg):
        """The trainer's one-batch lookahead: the next batch's index-only work (bitmaps, scatter plan, id lists) on the
        engine's side stream."""
        if self.fused_step_available():
            self._fused_engine().prefetch(users, pos, neg)


class _PackedPanel(torch.autograd.Function):
    """(user_weight, item_weight) -> the [n, d] panel they both live in, without copying."""

    @staticmethod
    def forward(ctx, user_w, item_w, storage):
        ctx.U = user_w.shape[0]
        return storage.view(storage.shape)

    @staticmethod
    def backward(ctx, g):
        return g[: ctx.U], g[ctx.U:], None


class PackedRecommender(nn.Module):
    #: number of propagation layers (0 = plain matrix factorisation) and whether layer 0 is averaged in
    n_layers = 0
    include_layer0 = True

    def __init__(self, config, dataset, device):
        super().__init__()
        self.config, self.dataset, self.device = config, dataset, device
        self.reg_lambda = float(config["reg_lambda"])
        d = int(config["embedding_size"])
        # construction order fixes the torch RNG consumption: normal_(user), normal_(item),
        # then the two xavier calls (models/LightGCN.py:21-28)
        self.user_embedding = nn.Embedding(num_embeddings=dataset.num_users, embedding_dim=d)
        self.item_embedding = nn.Embedding(num_embeddings=dataset.num_items, embedding_dim=d)
        nn.init.xavier_uniform_(self.user_embedding.weight, gain=1)
        nn.init.xavier_uniform_(self.item_embedding.weight, gain=1)
        self.activation = nn.Sigmoid()
        self.Graph = None
        self._storage = None
        self._engine = None
        self._eval_cache = None
        self._pack()

    # ------------------------------------------------------------------ packed storage
    def _pack(self):
        uw, iw = self.user_embedding.weight, self.item_embedding.weight
        U = uw.shape[0]
        storage = torch.cat([uw.data, iw.data]).contiguous()
        uw.data, iw.data = storage[:U], storage[U:]
        self._storage = storage
        self._engine = None
        self._eval_cache = None

    def _apply(self, fn, *a, **kw):
        out = super()._apply(fn, *a, **kw)
        self._pack()  # .to(device) / .float() re-create the tensors: restore the aliasing
        return out

    def _is_packed(self):
        uw, iw, st = self.user_embedding.weight, self.item_embedding.weight, self._storage
        return (st is not None and uw.data_ptr() == st.data_ptr() and uw.device == st.device
                and iw.data_ptr() == st.data_ptr() + uw.numel() * 4)

    def ego_panel(self):
        """Differentiable [n, d] view of both tables."""
        if not self._is_packed():
            self._pack()
        return _PackedPanel.apply(self.user_embedding.weight, self.item_embedding.weight, self._storage)

    def train(self, mode=True):
        self._eval_cache = None  # weights may change: drop the cached evaluation panels
        return super().train(mode)

    # ------------------------------------------------------------------ graph
    def attach_graph(self, sp_mat):
        """Upload a scipy adjacency to the model's device as an ops.Graph."""
        from utility.utility_function import tools

        dev = torch.device(self.device)
        if dev.type != "cuda":
            raise RuntimeError("%s needs an MI355X: device is %s and idgrec_amd has no CPU path "
                               "(torch.cuda.is_available() = %s)." % (type(self).__name__, dev, torch.cuda.is_available()))
        self.Graph = tools.convert_sp_mat_to_graph(sp_mat, dev)
        return self.Graph

    # ------------------------------------------------------------------ fused paths
    def engine(self):
        if self._engine is None or self._engine.params.data_ptr() != self._storage.data_ptr():
            if not self._is_packed():
                self._pack()
            ops._require_device(self._storage)
            self._engine = PropagationEngine(self.Graph if self.n_layers > 0 else None, self.dataset.num_users,
                                             self.dataset.num_items, self._storage.shape[1], self.n_layers,
                                             include_layer0=self.include_layer0, reg_lambda=self.reg_lambda,
                                             params=self._storage)
        return self._engine

    #: models whose training loss is exactly [bpr, reg] over the mean-propagated panel set this
    supports_fused_step = False
    #: entries of the loss vector a fused step writes ([bpr, reg] + the model's own terms)
    n_fused_losses = 2
    #: widths the row-restricted / masked / Adam-epilogue forms of the tiled SpMM exist for (idg_graph.hip,
    #: spmm_dispatch): the fused step is built from them, any other width trains through forward() + autograd
    FUSED_WIDTHS = (32, 64, 128, 256, 512)

    def fused_step_available(self):
        """True when the trainer may use fused_train_step(): the model offers one, lives on the GPU, and — if it
        propagates — its embedding width is one the fused kernels are instantiated for.  embedding_size = 48 or 100
        (values the reference's users run) then train through the generic-width kernels under autograd instead of
        failing in the first step."""
        if not self.supports_fused_step or self._storage is None or not self._storage.is_cuda:
            return False
        return self.n_layers == 0 or int(self._storage.shape[1]) in self.FUSED_WIDTHS

    def fused_loss_and_grad(self, users, pos, neg, loss_out=None):
        """Losses [bpr, reg_lambda*reg] (device tensor) and d(sum)/d(weights) written into the
        two parameters' .grad — the work of forward() + backward() without an autograd graph."""
        eng = self.engine()
        self._eval_cache = None
        loss = eng.loss_and_grad(users, pos, neg, loss_out)
        U = self.dataset.num_users
        self.user_embedding.weight.grad = eng.grad[:U]
        self.item_embedding.weight.grad = eng.grad[U:]
        return loss

    def _packed_adam(self, optimizer):
        """The hand-off of a fused step to `optimizer`: (param group, user state, item state, (exp_avg, exp_avg_sq) panels),
        or None — nothing done — unless it is an idgrec_amd.ops.Adam over exactly this model's two packed tables whose two
        step counters agree.  Its state (step, exp_avg, exp_avg_sq) stays the single source of truth: the moments are
        re-homed once into packed [n, d] panels that the state entries then view."""
        uw, iw = self.user_embedding.weight, self.item_embedding.weight
        group = adam_group_over(optimizer, [uw, iw])
        if group is None:
            return None
        if not self._is_packed():
            self._pack()
        U = self.dataset.num_users
        st_u, st_i = optimizer.state[uw], optimizer.state[iw]
        packed, homes = getattr(self, "_packed_moments", (None, None))
        # (an optimizer whose state is not in the panels yet gets FRESH ones: moments another optimizer left are not its own)
        if (packed is None or packed[0].device != self._storage.device or not st_u or not st_i
                or st_u["exp_avg"].data_ptr() != homes[0][1].data_ptr() or st_i["exp_avg_sq"].data_ptr() != homes[1][2].data_ptr()):
            m, v = torch.zeros_like(self._storage), torch.zeros_like(self._storage)
            packed, homes = self._packed_moments = (m, v), [(uw, m[:U], v[:U]), (iw, m[U:], v[U:])]
        if adopt_adam_state(optimizer, homes) is None:
            return None
        return group, st_u, st_i, packed

    def fused_train_step(self, users, pos, neg, loss_out, optimizer):
        """forward + backward + optimizer.step() as ONE chain of kernels (Adam is applied in the epilogue of the
        last backward product), in the state of `optimizer` as _packed_adam hands it over.  Returns False — nothing
        done — when it does not."""
        adam = self._packed_adam(optimizer)
        if adam is None:
            return False
        group, st_u, st_i, packed = adam
        uw, iw = self.user_embedding.weight, self.item_embedding.weight
        U = self.dataset.num_users
        eng = self.engine()
        eng.exp_avg, eng.exp_avg_sq = packed
        eng.lr, eng.betas, eng.eps = float(group["lr"]), tuple(group["betas"]), float(group["eps"])
        eng.step_count = int(st_u["step"])
        self._eval_cache = None
        # the update consumes the gradient inside the last product's epilogue; the panel is written out only on request
        # (model.keep_fused_grad = True): otherwise .grad reads None after a fused step, as after zero_grad(set_to_none=True)
        eng.store_grad = bool(getattr(self, "keep_fused_grad", False))
        eng.train_step(users, pos, neg, loss_out)
        st_u["step"] = st_i["step"] = eng.step_count
        if eng.store_grad:
            uw.grad, iw.grad = eng.grad[:U], eng.grad[U:]
        else:
            uw.grad = iw.grad = None
        return True

    def prefetch_batch(self, users, pos, neg):
        """One-batch lookahead for the fused step (row bitmap + scatter plan on the side stream; the plan alone for
        MFBPR)."""
        if self.fused_step_available():
            self.engine().prefetch(users, pos, neg)

    def final_panels(self):
        """(users [U,d'], items [I,d']) used for scoring, cached while the weights are frozen.
        Default: the layer-mean propagation of the packed panel; encoders with their own
        aggregate() (NGCF) override `_eval_panels`."""
        if self._eval_cache is None:
            self._eval_cache = self._eval_panels()
        return self._eval_cache

    def _eval_panels(self):
        fin = self.engine().propagate(force=True)
        U = self.dataset.num_users
        return fin[:U], fin[U:]

    def get_rating_for_test(self, user):
        """sigmoid(E_u[user] . E_i^T) as a dense [B, num_items] matrix (models/LightGCN.py:74-80)."""
        with torch.no_grad():
            ue, ie = self.final_panels()
            return ops.score_dense(ue, ie, user.long(), apply_sigmoid=True)

    #: ranks one call of the fused scoring / top-K entry point returns (idg_score_topk_f32: one pass per 64 ranks)
    FUSED_TOPK_MAX = 1024

    def topk_for_test(self, user, k):
        """Top-k unseen items per user without materialising the rating matrix (k up to FUSED_TOPK_MAX; beyond that —
        torch.topk takes any k <= num_items, batch_test.py:68 — the dense rating matrix, the reference's mask and
        torch.topk, batch by batch)."""
        with torch.no_grad():
            ue, ie = self.final_panels()
            ip, ix = self.dataset.train_csr_on(ue.device)
            user = user.long()
            if k <= self.FUSED_TOPK_MAX:
                return ops.score_topk(ue, ie, user, k, ip, ix, apply_sigmoid=True)
            out = []
            for lo in range(0, user.shape[0], 256):
                u = user[lo:lo + 256]
                rating = ops.score_dense(ue, ie, u, apply_sigmoid=True)
                cnt = ip[u + 1] - ip[u]
                rows = torch.repeat_interleave(torch.arange(u.shape[0], device=u.device), cnt)
                cols = torch.cat([ix[int(a):int(b)] for a, b in zip(ip[u].tolist(), ip[u + 1].tolist())]).long() if int(cnt.sum()) else rows
                rating[rows, cols] = -1
                out.append(torch.topk(rating, k=k)[1])
            return torch.cat(out)


class LayerChainRecommender(PackedRecommender):
    """LightGCN mean + BPR + contrastive terms that read individual layers' outputs and whose gradients reach every row of
    both tables (CGCL, NCL).  The fused step keeps every layer: K products with the running layer sum in their epilogue, the
    fused BPR on the mean, the subclass's contrastive calls adding into one gradient panel per layer they read, the backward
    chain g_k = A g_(k+1) + g_mean / (K + 1) + g_ssl_k, and a dense Adam step of the packed panel.  A subclass sets n_layers,
    attaches the graph and states `ssl_layers`, `ssl_parts` and `_ssl_raw`."""
    supports_fused_step = True
    #: the layers whose output carries a contrastive gradient panel; layer 0 is always one (the regulariser's gradient lands there)
    ssl_layers = None
    #: shape of the zeroed float32 scratch _ssl_raw's calls write their loss terms to
    ssl_parts = None
    _buf = None

    def _ssl_raw(self, E, G, users, pos, parts, loss_out):
        """Issue the contrastive calls: E = [E0, .., EK], G = {layer: its gradient panel, added into}, parts = the zeroed
        scratch; writes loss_out[2:]."""
        raise NotImplementedError

    def _layers(self):
        """([E0, E1, .., EK], their mean [n, d])."""
        layers = [self.ego_panel()]
        for _ in range(self.n_layers):
            layers.append(ops.spmm(self.Graph, layers[-1]))
        return layers, torch.stack(layers, dim=1).mean(dim=1)

    def aggregate(self):
        """(users [U,d], items [I,d], [E0, E1, .., EK]): the layer mean and every layer's output."""
        layers, final = self._layers()
        users, items = torch.split(final, [self.dataset.num_users, self.dataset.num_items])
        return users, items, layers

    def _step_buffers(self):
        st = self._storage
        if self._buf is None or self._buf["key"] != (st.data_ptr(), st.device):
            K = self.n_layers
            new = lambda: torch.empty_like(st)  # noqa: E731
            self._buf = dict(key=(st.data_ptr(), st.device), E=[None] + [new() for _ in range(K)], S=new(), final=new(),
                             g_final=new(), G={k: new() for k in self.ssl_layers}, chain=[new(), new()], grad=None,
                             parts=torch.empty(self.ssl_parts, dtype=torch.float32, device=st.device))
        return self._buf

    def fused_loss_and_grad(self, users, pos, neg, loss_out=None):
        """The n_fused_losses losses (device tensor) and d(sum) / d(weights) in the two parameters' .grad, as one fixed chain
        of library calls."""
        if not self._is_packed():
            self._pack()
        st = self._storage
        U, K = self.dataset.num_users, self.n_layers
        users, pos, neg = (t.long().contiguous() for t in (users, pos, neg))
        buf = self._step_buffers()
        self._eval_cache = None
        if loss_out is None:
            loss_out = torch.empty(self.n_fused_losses, dtype=torch.float32, device=st.device)
        E, G = buf["E"], buf["G"]
        E[0] = st
        # layers 1..K and their mean: the running sum rides in the product's epilogue
        for k in range(1, K + 1):
            last = k == K
            ops.spmm_ex_raw(self.Graph, E[k - 1], Y=E[k], sum_in=E[0] if k == 1 else buf["S"],
                            sum_out=buf["final"] if last else buf["S"], div=float(K + 1) if last else 1.0)
        for t in (buf["g_final"], *G.values()):
            t.zero_()
        # BPR on the mean; the regulariser's gradient lands with layer 0's
        ops.bpr_fused_raw(buf["final"], st, users, pos, neg, U, self.reg_lambda, buf["g_final"], G[0], loss=loss_out[0:2])
        self._ssl_raw(E, G, users, pos, buf["parts"].zero_(), loss_out)
        # g_k = A g_(k+1) + g_final / (K + 1) + g_ssl_k, from the last layer down (g_ssl_k = 0 for a layer without a panel)
        share = 1.0 / (K + 1)
        cur = buf["chain"][K % 2]
        if K in G:
            ops.lincomb_raw(cur, G[K], 1.0, buf["g_final"], share)
        else:
            ops.lincomb_raw(cur, buf["g_final"], share)
        for k in range(K - 1, -1, -1):
            if k in G:
                add = G[k]
                ops.lincomb_raw(add, add, 1.0, buf["g_final"], share)
            else:
                add = buf["S"]
                ops.lincomb_raw(add, buf["g_final"], share)
            nxt = buf["chain"][k % 2]
            self.Graph.spmm_raw(cur, addend=add, out=nxt)
            cur = nxt
        buf["grad"] = cur
        self.user_embedding.weight.grad = cur[:U]
        self.item_embedding.weight.grad = cur[U:]
        return loss_out

    def fused_train_step(self, users, pos, neg, loss_out, optimizer):
        """fused_loss_and_grad + the dense Adam step of the packed panel (the table gradients reach every row), in the state
        of `optimizer` as _packed_adam hands it over.  False — nothing done — when it does not."""
        adam = self._packed_adam(optimizer)
        if adam is None:
            return False
        group, st_u, st_i, (m, v) = adam
        self.fused_loss_and_grad(users, pos, neg, loss_out)
        step = int(st_u["step"]) + 1
        b1, b2 = group["betas"]
        ops.adam_step_raw(self._storage, self._buf["grad"], m, v, group["lr"], step, b1, b2, group["eps"])
        st_u["step"] = st_i["step"] = step
        if not getattr(self, "keep_fused_grad", False):
            self.user_embedding.weight.grad = self.item_embedding.weight.grad = None
        return True

    def prefetch_batch(self, users, pos, neg):
        """Nothing to prepare ahead: the step's index work is inside its calls."""
