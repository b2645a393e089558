"""User-row-sharded LightGCN training step across the GPUs of one node.

The reference is single-device (models/LightGCN.py:36-72, utility/utility_train/trainer.py:36-56); this is new
functionality whose oracle is the single-GPU result.  Rank g owns a contiguous, nnz-balanced block of users: their
embedding rows (and Adam state), the rows R_g of the normalised interaction matrix (U_g x I) and the transposed block
R_g^T (I x U_g) — both with the GLOBAL d^-1/2 scaling, so the stacked blocks equal the single-GPU adjacency.  The item
TABLE is replicated (every rank gathers from all of it); its Adam state and its update are not: each rank owns 1/N of the
item rows.

One propagation layer:      X_U[g] <- R_g . X_I                           (local)
                            X_I    <- sum over ranks of R_g^T . X_U[g]    (RCCL over xGMI)
The item-side product of a layer needs local user rows only and is launched first, slice by slice, each slice's
collective right behind it on the communicator's stream; the user-side product is what waits for the previous layer's
exchange.  Only the exchanges whose consumers read every row move the [I, d] panel (K = 3: forward layer 1, the second
backward product, and the last backward product as a reduce-scatter); the others move the rows a batch touches.  After
the reduce-scatter each rank finishes the gradient and applies Adam for ITS item rows and all-gathers the updated rows
under the next step's first product, so the ranks' item tables are bit-identical by construction.

The layer loop names no concrete class: it talks to `kernels` and `comm`, the two interfaces written out in __init__.py.
"""
import numpy as np


# --------------------------------------------------------------------------- the step
class GlobalBatch:
    """Index-only description of ONE global batch as one rank sees it (built on the host by ShardedEngine.make_batch
    from the batch's global ids; every array lives where the kernels want it).  B triples; triple t owns guest row t.
      pos, neg   int64 [B]  global item ids
      own_src    int64 [B]  local id of triple t's user if this rank owns it, else -1 (fills the guest rows)
      head_dst   int64 [B]  the same id for the FIRST owned occurrence of a user in the batch, else -1
      nxt        int64 [B]  batch position of the next occurrence of triple t's user, -1 at the end of its chain
      own_users  int64 [B_g]  local ids of the owned triples' users: the user rows this rank's restricted products have
                 to produce / may gather from
      items      int64 [n_items <= 2B]  the batch's distinct item ids, ascending: the only item rows of the LAST forward
                 layer anybody reads (the BPR loss gathers pos / neg rows) — what that layer's exchange carries
      touched_bound  host int or None: an upper bound of the number of item rows the batch touches (its own items + the
                 items its users interacted with) computed from the GLOBAL user degrees — the same number on every rank,
                 known before the step: the touched-item exchanges are sized by it and need no host read-back"""
    __slots__ = ("B", "pos", "neg", "own_src", "head_dst", "nxt", "own_users", "n_owned", "key", "items", "n_items",
                 "touched_bound")
    _next_key = 0


class ShardedEngine:
    """One rank's share of the LightGCN step (models/LightGCN.py:36-72 + utility/utility_train/trainer.py:42-56 cut by
    user rows; any number of propagation layers, GCN_layer in configure/LightGCN.txt:12).  Arrays are whatever `kernels`
    allocates (torch CUDA tensors in the product).

    Layout.  Every local panel has rows [0, U_g) = this rank's users, [U_g, U_g + B) = B GUEST rows (row U_g + t carries
    triple t's user, whoever owns it), then ALL items padded to I_p rows ([U_g + B, U_g + B + I_p)).  The item rows are cut
    into S slices (the same cuts on every rank; every slice a multiple of the world size long, the last one padded), and
    rank r OWNS the r-th N-th of every slice: it holds the Adam moments of those item rows only.

    What is exact and what is exchanged.  The batch is GLOBAL (every rank sees all B triples, as the single-device step
    does): after the forward propagation the owners copy the batch users' final and ego rows into the guest rows, two
    all-reduces of [B, d] (x + 0 + ... + 0: exact) hand them to every rank, and every rank evaluates the WHOLE batch's
    BPR loss — so the loss and the item-side gradient g_I are complete and bit-identical on every rank without any
    [I, d] exchange, and the user-side gradient rows flow back from the guest rows to their owners' rows (chains in batch
    order).  Nothing of size [n, d] is ever zero-filled: BPR and the chain mover STORE the rows they reach, and every
    consumer reads gradient panels through the batch's row bitmaps (kernels.prepare).
    Per training step at K = 3: forward layer 1 and the second backward product travel as sliced all-reduces of the
    [I, d] panel; forward layer K - 1 and the first backward product as the item rows the batch's users touch (agreed
    through an [I] flag vector: _agree_touched_items); the last forward layer as the batch's <= 2B item rows; and the
    LAST backward product as a reduce-scatter: each rank finishes the gradient and applies Adam for the item rows it
    owns (idg_grad_tail_adam_f32) and the UPDATED rows go round by an all-gather that runs under the next step's first
    item-side product (which needs the local user rows only).  No O(I d) work is replicated: the only replicated
    per-rank work is O(B d) (loss, guest rows) and the [I] flag vector."""

    def __init__(self, kernels, comm, ui_csr, iu_csr, n_local_users, num_items, dim, n_layers, include_layer0=True,
                 reg_lambda=1e-4, lr=1e-3, batch_sparsity=True, batch_size=1024, user_lo=0, n_slices=None, item_cuts=None,
                 live_rows_cap=None, live_rows_min_bytes=64 << 20, store_grad=True, global_user_degree=None):
        """batch_sparsity: use the batch's row bitmaps (kernels.prepare) — restricted products, stored gradient rows, no
        fills; False = every product dense over zero-filled gradient panels (the plain form, kept as an A/B check).
        batch_size: capacity of the guest rows (the global batch size).  user_lo: global id of this rank's first user.
        n_slices: row slices of R_g^T whose collectives overlap the following slices' products (default: 4 once the
        item panel reaches 256 MB, else 1); item_cuts: the slices' row bounds — the same on every rank; default: equal
        row counts (callers that know the global item degrees pass entry-balanced cuts).  live_rows_cap: rows of the
        compact buffer of the touched-item exchanges (default 64 per triple; the same on every rank);
        live_rows_min_bytes: item panels smaller than this skip the touched-item forms (tests pass 0).
        store_grad: keep the finished gradient in G — the user rows and the OWNED item rows (tests read it; the step
        does not: without it the last products feed Adam and write no gradient panel).
        global_user_degree: int array [U] of EVERY user's number of train items (the same array on every rank).  With it
        the number of item rows a batch touches is bounded on the host (make_batch), the touched-item exchanges move that
        many rows through a fixed-capacity id list built on the device, and the step has no host synchronisation; without
        it the ranks read the list's length back (one synchronisation per step)."""
        self.k, self.comm = kernels, comm
        self.world, self.rank = int(getattr(comm, "world", 1)), int(getattr(comm, "rank", 0))
        self.batch_sparsity = bool(batch_sparsity)
        self._prepared = {}
        self.Ug, self.I, self.d, self.K = int(n_local_users), int(num_items), int(dim), int(n_layers)
        if not 1 <= self.K <= 15:
            raise ValueError("ShardedEngine: 1 <= n_layers <= 15; got %d" % self.K)
        self.user_degree = None if global_user_degree is None else np.asarray(global_user_degree, dtype=np.int64)
        self.B, self.lo = int(batch_size), int(user_lo)
        self.c0 = 1 if include_layer0 else 0
        self.cnt = float(self.K + self.c0)
        self.reg_lambda, self.lr = float(reg_lambda), float(lr)
        self.store_grad = bool(store_grad)
        self.G_ui = kernels.make_graph(*ui_csr, self.Ug, self.I)
        if n_slices is None:
            n_slices = 4 if self.I * self.d * 4 >= (256 << 20) else 1
        iu_ptr, iu_idx, iu_val = iu_csr
        iu_ptr = np.asarray(iu_ptr, dtype=np.int64)
        if item_cuts is None:
            item_cuts = np.linspace(0, self.I, max(1, min(int(n_slices), self.I)) + 1).astype(np.int64)
        cuts = np.asarray(item_cuts, dtype=np.int64).copy()
        # inner cuts on multiples of 32 x world rows: a slice's share of an item-row bitmap starts on a word boundary and
        # every inner slice divides evenly among the ranks (the rounding is a function of the cuts and the world size
        # alone, so the ranks agree on it)
        q = 32 * self.world
        cuts[1:-1] = np.minimum((cuts[1:-1] + q // 2) // q * q, self.I // q * q)
        cuts = np.maximum.accumulate(cuts)
        assert cuts[0] == 0 and cuts[-1] == self.I and (np.diff(cuts) >= 0).all(), "item_cuts must tile [0, I]"
        # slices: (graph, r0, r1, r1p) — rows [r0, r1) exist, [r0, r1p) is the slice's share of the padded panel
        self.slices = []
        for r0, r1 in zip(cuts[:-1], cuts[1:]):
            r0, r1 = int(r0), int(r1)
            if r1 == r0:
                continue
            e0, e1 = int(iu_ptr[r0]), int(iu_ptr[r1])
            g = kernels.make_graph(iu_ptr[r0:r1 + 1] - e0, iu_idx[e0:e1], iu_val[e0:e1], r1 - r0, self.Ug)
            self.slices.append([g, r0, r1, r1])
        last = self.slices[-1]
        last[3] = last[1] + -(-(last[2] - last[1]) // self.world) * self.world
        self.slices = [tuple(sl) for sl in self.slices]
        self.Ip = self.slices[-1][3]
        # the blocks of item rows this rank owns: (first row, rows, offset into the compact moment arrays)
        self.own, off = [], 0
        for _, r0, _, r1p in self.slices:
            c = (r1p - r0) // self.world
            self.own.append((r0 + self.rank * c, c, off))
            off += c
        n = self.Ug + self.B + self.Ip
        z = kernels.zeros
        self.P, self.G = z((n, dim)), z((n, dim))
        self.FIN = z((n, dim))
        self.GF = z((n, dim))   # d loss / d FIN
        self.MU, self.VU = z((self.Ug, dim)), z((self.Ug, dim))        # Adam moments: the owned user rows ...
        self.MI, self.VI = z((max(off, 1), dim)), z((max(off, 1), dim))  # ... and the owned item rows (1/N of the table)
        # 24-bit panel exchange (Packed24Comm): the replicated item table then holds 24-bit values on EVERY rank (the owner's
        # copy too: replicas stay bit-identical), so the owner keeps the fp32 MASTER of its rows here — Adam updates the
        # master, the all-gather sends it packed.  Filled from the table by the first training step.
        self.packed = bool(getattr(comm, "packed", False))
        self.by_blocks = bool(getattr(comm, "by_blocks", False))  # (an explicit exchange, packed or not: slices by rank blocks)
        self.MP = z((max(off, 1), dim)) if self.packed else None
        self._master_ready = False
        self.XU = [z((self.Ug, dim)) for _ in range(max(self.K - 1, 1))]
        self.XI = [z((self.Ip, dim)) for _ in range(self.K)]
        # more than three earlier layers do not fit one epilogue (sum_in .. sum_in3): from K = 4 on the user-side layer sum
        # is carried from product to product (sum_in -> sum_out, left to right as torch.mean(torch.stack(...)) adds)
        self.SU = z((self.Ug, dim)) if self.K + self.c0 > 4 else None
        self.CI = z((2 * self.B, dim))  # the batch's item rows, compact (last forward layer)
        # flags of the item rows some rank's batch users touch, and those rows, compact (up to 64 per triple)
        self.FL = z((self.I,))
        self.live_rows_min_bytes = int(live_rows_min_bytes)
        default_cap = (128 if self.user_degree is not None else 64) * self.B  # (a bound is looser than a count)
        self.CS = z((max(1, min(self.I, default_cap if live_rows_cap is None else int(live_rows_cap))), dim))
        self._touch_misses, self._touch_skip = 0, 0   # consecutive overflows of CS; steps left before asking again
        self.timeline = None  # StepTimeline while instrumented steps run (bench.py, after the timed region)
        self.loss = z((2,))
        self.guest_ids = kernels.to_device(np.arange(self.Ug, self.Ug + self.B, dtype=np.int64))
        # views handed to the kernels every step, made once (slicing a tensor costs the host ~1.5 us)
        self.P_u, self.P_i = self._u(self.P), self._i(self.P)
        self.FIN_u, self.FIN_i = self._u(self.FIN), self._i(self.FIN)
        self.GF_u, self.GF_i = self._u(self.GF), self._i(self.GF)
        self.G_u, self.G_i = self._u(self.G), self._i(self.G)
        self._views = {}
        self._all_item_ids = None
        self._all_items_bits = None
        self._ag = []          # all-gathers of the updated item rows still in flight (waited before P_I is read again)
        self.touched_items = None
        self.step_count = 0

    def _u(self, a):
        return a[: self.Ug]

    def _guest(self, a, count=None):
        return a[self.Ug: self.Ug + (self.B if count is None else count)]

    def _i(self, a):
        return a[self.Ug + self.B:]

    def _slice_rows(self, panel_i, j, padded=False):
        """Rows of slice j of an item-row panel ([I_p, d]); padded: up to the slice's share of the padding."""
        key = (id(panel_i), j, padded)
        v = self._views.get(key)
        if v is None:
            _, r0, r1, r1p = self.slices[j]
            v = self._views[key] = (panel_i, panel_i[r0:(r1p if padded else r1)])  # (keeps the panel alive: id() stays its)
        return v[1]

    def item_rows(self, a):
        """The real item rows of a local panel (without the padding)."""
        return a[self.Ug + self.B: self.Ug + self.B + self.I]

    # ---- index-only preparation of a global batch (host)
    def make_batch(self, users, pos, neg):
        """users: GLOBAL user ids [B' <= B] (numpy), pos / neg: global item ids."""
        users = np.asarray(users, dtype=np.int64)
        Bc = len(users)
        assert 0 < Bc <= self.B, "batch of %d triples, engine built for up to %d" % (Bc, self.B)
        local = users - self.lo
        owned = (local >= 0) & (local < self.Ug)
        own_src = np.where(owned, local, -1)
        # chains over the occurrences of one user, in batch order (stable sort by user, then by position)
        order = np.argsort(users, kind="stable")
        su = users[order]
        nxt = np.full(Bc, -1, dtype=np.int64)
        same = su[1:] == su[:-1]
        nxt[order[:-1][same]] = order[1:][same]
        first = np.ones(Bc, dtype=bool)
        first[order[1:][same]] = False
        gb = GlobalBatch()
        to = self.k.to_device
        gb.B = Bc
        gb.pos, gb.neg = to(np.asarray(pos, dtype=np.int64)), to(np.asarray(neg, dtype=np.int64))
        gb.own_src = to(own_src.astype(np.int64))
        gb.head_dst = to(np.where(owned & first, local, -1).astype(np.int64))
        gb.nxt = to(nxt)
        gb.n_owned = int(owned.sum())
        gb.own_users = to(local[owned].astype(np.int64))
        items = np.unique(np.concatenate([np.asarray(pos, dtype=np.int64), np.asarray(neg, dtype=np.int64)]))
        gb.items, gb.n_items = to(items), len(items)
        gb.touched_bound = None
        if getattr(self, "user_degree", None) is not None:
            # every distinct batch user contributes at most its degree, the batch at most its own items: >= the union
            gb.touched_bound = int(min(self.I, self.user_degree[su[np.concatenate([[True], ~same])]].sum() + len(items)))
        GlobalBatch._next_key += 1
        gb.key = GlobalBatch._next_key  # (a counter: id(gb) can come back after a skipped batch is collected)
        return gb

    # ---- collectives
    def _wait(self, works):
        for w in works:
            self.comm.wait(w)

    def _wait_item_table(self):
        """The previous step's all-gathers of the updated item rows: P_I is whole again after them."""
        self._wait(self._ag)
        self._ag = []

    def _item_side(self, X_u, Y_i, out_bits=None, x_rows=None, addend=None, mask=None, reduce="all", tag="panel"):
        """Y_i[slice] = R_g^T[slice] . X_u (+ addend, on rank 0 only: the ranks' partials are summed), slice by slice;
        each slice's collective is issued as soon as the slice exists, so it runs under the following slices' products
        and under whatever the caller launches next.  reduce: "all" = all-reduce of the slice, "scatter" = reduce-scatter
        (this rank keeps its own block of the slice), None = no exchange (the caller moves rows).  Returns the works."""
        k, works = self.k, []
        add = addend if self.rank == 0 else None
        # packed exchange: a slice whose partial goes straight into an all-reduce / reduce-scatter is written PACKED by the
        # product itself, into the exchange's send buffer (nobody reads the fp32 partial: the sum overwrites it)
        target = getattr(self.comm, "packed_target", None) if (self.packed and reduce in ("all", "scatter") and out_bits is None) else None
        for j, (g, r0, r1, r1p) in enumerate(self.slices):
            y = self._slice_rows(Y_i, j)
            y24 = target(self._slice_rows(Y_i, j, padded=True), (r1 - r0) * self.d) if target is not None else None
            k.spmm(g, X_u, Y=None if y24 is not None else y, addend=None if add is None else self._slice_rows(add, j),
                   mask=None if (add is None or mask is None) else k.bits_from(mask, r0),
                   out_rows=None if out_bits is None else k.bits_from(out_bits, r0), x_rows=x_rows,
                   **({"Y24": y24} if y24 is not None else {}))
            if reduce == "all":
                self.comm.tag, self.comm.slice = tag, j
                # (the packed exchange cuts a slice into one block per rank: the padded view — its padding rows are zero)
                works.append(self.comm.all_reduce_async(self._slice_rows(Y_i, j, padded=True) if self.by_blocks else y))
            elif reduce == "scatter":
                self.comm.tag, self.comm.slice = tag, j
                works.append(self.comm.reduce_scatter_async(self._slice_rows(Y_i, j, padded=True)))
        self.comm.slice = None
        return works

    def _sum_rows(self, panel, rows, tag="rows"):
        """all-reduce of the panel's rows `rows` = (ids, n) through the compact buffer (synchronous: small).  ids may
        repeat its last entry (a list padded to a host-side bound): the repeated row is gathered, summed and written
        back more than once, with the same value."""
        ids, n = rows
        self.k.gather_rows(self.CS[:n], panel, ids)
        self.comm.tag = tag
        self.comm.wait(self.comm.all_reduce_async(self.CS[:n]))
        self.k.scatter_rows(panel, ids, self.CS[:n])

    def _agree_touched_items(self, prep, gb):
        """The item rows a training batch touches beyond its own positives / negatives: the items its USERS interacted
        with.  Forward layer K - 1 is read there only (by the last user-side product, restricted to the batch's users,
        and by FIN at the batch's items) and the first backward product's partials are zero elsewhere, so both travel as
        these rows instead of the [I, d] panel, and the products around them are restricted to them.
        One rank marks the bitmap locally.  Several ranks flag the items of the batch users they own
        (idg_graph_flag_cols over their block of R), add the batch's items and sum the flags ([I] floats: 20 MB at
        configs[4]); the ascending id list is built ON THE DEVICE into a list of gb.touched_bound slots (a host-side
        bound from the global user degrees, the same on every rank; slots past the last id repeat it:
        idg_flags_compact_f32) — no host synchronisation.  Without the degrees (global_user_degree=None) the list's
        length is read back: one synchronisation per step, and after three consecutive batches that overflow the
        compact buffer the engine stops asking for 64 steps.
        Sets prep.touched (bitmap) and self.touched_items = (ids, n) (several ranks) or leaves both None: K < 2, a panel
        too small to be worth it, or more rows than the compact buffer holds."""
        self.touched_items = None
        if prep is None or self.K < 2 or self.I * self.d * 4 < self.live_rows_min_bytes:
            return
        k = self.k
        if self.world == 1:
            k.touched_local(self, prep, gb)
            return
        cap = self.CS.shape[0]
        tl = self.timeline
        if gb.touched_bound is not None:
            if gb.touched_bound > cap:   # known before anything is launched, and the same on every rank
                return
            n = min(cap, -(-gb.touched_bound // 256) * 256)  # (whole 256-row blocks: fewer distinct collective sizes)
            k.flag_touched_items(self, prep, gb, self.FL)
            self.comm.tag = "flags"
            self.comm.wait(self.comm.all_reduce_async(self.FL))
            ids = k.compact_ids(self.FL, n)
            self.touched_items = (ids, n)
            k.touched_from_ids(self, prep, ids, n)
            return
        if self._touch_skip > 0:
            self._touch_skip -= 1
            return
        k.flag_touched_items(self, prep, gb, self.FL)
        self.comm.tag = "flags"
        self.comm.wait(self.comm.all_reduce_async(self.FL))
        t0 = tl.host_sync_begin() if tl is not None else None
        ids, n = k.nonzero_ids(self.FL)
        if tl is not None:
            tl.host_sync_end(t0)
        if n == 0 or n > cap:
            self._touch_misses += 1
            if self._touch_misses >= 3:
                self._touch_misses, self._touch_skip = 0, 64
            return
        self._touch_misses = 0
        self.touched_items = (ids, n)
        k.touched_from_ids(self, prep, ids, n)

    # ---- forward: FIN = mean_k A^k P at the rows the caller reads (a training step: the batch's; evaluation: all)
    def propagate(self, prep=None, gb=None):
        """Layer k: X_I(k) = sum over ranks of R_g^T X_U(k-1),  X_U(k) = R_g X_I(k-1).  The item-side partial of a layer
        needs only LOCAL user rows, so it is launched before the previous layer's exchange is waited for; the user-side
        product is what waits.  With a batch (gb) the step reads FIN at the batch's rows only, and each layer is produced
        on the rows its consumers read: layer K at the batch's users / items, layer K - 1 at the users near the batch's
        items / the touched items (kernels.prepare and _agree_touched_items), earlier layers everywhere.  The layer mean
        is formed once, by the last product's epilogue (users) and by one rows kernel (the batch's items), in
        torch.mean(torch.stack(...))'s left-to-right order.  Evaluation calls propagate() without a batch: every row."""
        k, K, c0, cnt = self.k, self.K, self.c0, self.cnt
        P_u, P_i, fin_u, fin_i = self.P_u, self.P_i, self.FIN_u, self.FIN_i
        train = gb is not None
        self.touched_items = None
        touched = near = None
        items_bits = prep.items if (train and prep is not None) else None
        users_bits = prep.own_users if (train and prep is not None) else None
        pending = []  # collectives of the previous layer's item side
        # the user-side layer sum: at most three earlier terms fit the last product's epilogue; beyond that (K + c0 > 4)
        # every product adds its output to the running sum SU (sum_in -> sum_out, the left-to-right order of
        # torch.mean(torch.stack(...)), as idg_propagate_mean_f32 does on one device) and the last one divides
        chain = self.SU is not None
        acc = [P_u] if c0 else []  # terms not yet folded into SU (chain form)
        for layer in range(1, K + 1):
            last, pre = layer == K, layer == K - 1
            if pre and train:
                # agreed as late as possible: the flag exchange queues behind the collectives already issued (the previous
                # step's all-gathers, layer 1's all-reduce), which the products launched so far overlap
                self._agree_touched_items(prep, gb)
                touched = getattr(prep, "touched", None) if prep is not None else None
                near = getattr(prep, "near", None) if touched is not None else None
            xu_prev = P_u if layer == 1 else self.XU[layer - 2]
            xi_prev = P_i if layer == 1 else self.XI[layer - 2]
            xi_new = self.XI[layer - 1]
            # item side of this layer (input: local user rows)
            if last and train:
                works = self._item_side(xu_prev, xi_new, out_bits=items_bits, reduce=None)
                k.gather_rows(self.CI[:gb.n_items], xi_new, gb.items)
                self.comm.tag = "F%d.items" % layer
                works = [self.comm.all_reduce_async(self.CI[:gb.n_items])]
            elif pre and touched is not None:
                works = self._item_side(xu_prev, xi_new, out_bits=touched, reduce=None)
                if self.touched_items is not None:
                    self._sum_rows(xi_new, self.touched_items, tag="F%d.touched" % layer)
            else:
                works = self._item_side(xu_prev, xi_new, tag="F%d.panel" % layer)
            # user side (input: the previous layer's item rows, exchanged; layer 1: the item table itself)
            self._wait(pending)
            if layer == 1:
                self._wait_item_table()
            if last:
                terms = acc if chain else ([P_u] if c0 else []) + self.XU[: K - 1]
                k.spmm(self.G_ui, xi_prev, sums=terms, sum_out=fin_u, div=cnt, out_rows=users_bits)
            elif chain and acc:
                k.spmm(self.G_ui, xi_prev, Y=self.XU[layer - 1], sums=acc, sum_out=self.SU, out_rows=near if pre else None)
                acc = [self.SU]
            else:
                k.spmm(self.G_ui, xi_prev, Y=self.XU[layer - 1], out_rows=near if pre else None)
                if chain:
                    acc = [self.XU[layer - 1]]  # (no layer 0 in the mean: the sum starts with layer 1)
            pending = works
        self._wait(pending)
        # the layer mean at the item rows: the batch's (their last layer arrived as the compact row set), or all
        terms = ([P_i] if c0 else []) + self.XI[: K - 1]
        if train:
            k.layer_mean(fin_i, gb.items, terms, self.CI[:gb.n_items], cnt)
        else:
            if self._all_item_ids is None:
                self._all_item_ids = k.to_device(np.arange(self.I, dtype=np.int64))
            k.layer_mean(fin_i, self._all_item_ids, terms, self.XI[K - 1][: self.I], cnt)
        return self.FIN

    # ---- backward of the above given GF = d loss / d FIN (g_I complete on every rank, g_U at the owners' rows; live
    #      rows: the batch's), accumulated onto G (which holds the regulariser gradient at the same rows), Adam included
    def propagate_backward(self, prep, gb, adam_step):
        """Horner steps h <- A.h + g, then gE0 = (A.h + c0.g)/cnt.  In block form (A.h)_U = R_g h_I (local), (A.h)_I =
        sum over ranks of R_g^T h_U.  As in the forward pass the item-side partial of a step needs only the LOCAL h_U and
        is launched before the previous exchange is waited for.  Step 1's inputs live on the batch's rows, its outputs on
        the touched items / the near users; from step 2 on everything is dense.  The LAST step's item side ends in a
        reduce-scatter: this rank finishes the gradient and applies Adam for the item rows it owns, slice by slice as each
        slice's collective lands, and sends the updated rows round (all-gathers left in flight: _wait_item_table); its
        user side applies Adam to the owned user rows in the product's epilogue."""
        k, K, c0, cnt = self.k, self.K, self.c0, self.cnt
        g_u, g_i, G_u, G_i, P_i = self.GF_u, self.GF_i, self.G_u, self.G_i, self.P_i
        sparse = prep is not None
        users_bits = prep.own_users if sparse else None      # live rows of g_U / reg_U (the owned batch users)
        items_bits = prep.items if sparse else self._ones_items()  # live rows of g_I / reg_I (the batch's items)
        touched = getattr(prep, "touched", None) if sparse else None
        near = getattr(prep, "near", None) if touched is not None else None
        h_u, h_i = g_u, g_i
        live_u, live_i = users_bits, (items_bits if sparse else None)
        pending = []
        for step in range(1, K):
            t_i, t_u = self.XI[step - 1], self.XU[step - 1]
            first = step == 1 and touched is not None
            # item side: sum over ranks of R_g^T h_U, + g_I (added once: by rank 0's partial)
            if first:
                works = self._item_side(h_u, t_i, out_bits=touched, x_rows=live_u, addend=g_i, mask=items_bits, reduce=None)
                if self.touched_items is not None:
                    self._sum_rows(t_i, self.touched_items, tag="B%d.touched" % step)
            else:
                works = self._item_side(h_u, t_i, x_rows=live_u, addend=g_i, mask=items_bits if sparse else None,
                                        tag="B%d.panel" % step)
            # user side: R_g h_I + g_U
            self._wait(pending)
            k.spmm(self.G_ui, h_i, Y=t_u, addend=g_u, mask=users_bits, out_rows=near if first else None, x_rows=live_i)
            pending = works
            h_u, h_i = t_u, t_i
            live_u, live_i = (near, touched) if first else (None, None)
        # last step, scaled by 1 / cnt
        t_i = self.XI[K - 1]
        works = self._item_side(h_u, t_i, x_rows=live_u, reduce="scatter", tag="B%d.reduce_scatter" % K)
        self._wait(pending)
        adam = (self.P_u, self.MU, self.VU, self.lr, adam_step)
        if live_i is None:   # a dense launch: the owned users' Adam update rides in its epilogue
            k.spmm(self.G_ui, h_i, sums=[g_u] if c0 else [], sum_out=G_u, div=cnt, accumulate=True, mask=users_bits, adam=adam,
                   discard_grad=not self.store_grad)
        else:                # (K <= 2 with restricted inputs: the epilogue form needs the dense kernel)
            k.spmm(self.G_ui, h_i, sums=[g_u] if c0 else [], sum_out=G_u, div=cnt, accumulate=True, mask=users_bits,
                   x_rows=live_i)
            k.adam(self.P_u, G_u, self.MU, self.VU, self.lr, adam_step)
        # the owned item rows: finish the gradient, Adam, and send the updated rows round
        for j, (w, (o0, c, off)) in enumerate(zip(works, self.own)):
            self.comm.wait(w)
            blocks = self._own_blocks(j, t_i)
            if c > 0:
                k.item_tail(blocks[0], blocks[1], blocks[2], items_bits, o0, c0, cnt, self.store_grad, blocks[3],
                            blocks[4], blocks[5], self.lr, adam_step)
            self.comm.tag, self.comm.slice = "item_table.all_gather", j
            self._ag.append(self.comm.all_gather_async(self._slice_rows(P_i, j, padded=True), blocks[3]))
        self.comm.slice = None
        return self.G

    def _own_blocks(self, j, t_i):
        """The rows of slice j this rank owns, in (t, g, G, P, M, V)."""
        key = ("own", id(t_i), j)
        v = self._views.get(key)
        if v is None:
            o0, c, off = self.own[j]
            blk = slice(o0, o0 + c)
            # (packed exchange: Adam's parameter rows and the all-gather's source are the fp32 master, not the table's own copy)
            p_rows = self.MP[off:off + c] if self.packed else self.P_i[blk]
            v = self._views[key] = (t_i[blk], self.GF_i[blk], self.G_i[blk], p_rows, self.MI[off:off + c],
                                    self.VI[off:off + c], t_i)
        return v

    def _ones_items(self):
        if self._all_items_bits is None:
            self._all_items_bits = self.k.ones_bits(self.Ip)
        return self._all_items_bits

    def train_step(self, gb):
        """gb: a GlobalBatch from make_batch() — the same global batch on every rank."""
        k = self.k
        Bc = gb.B
        if self.packed and not self._master_ready:
            self._wait_item_table()
            for o0, c, off in self.own:
                if c > 0:
                    self.MP[off:off + c][...] = self.P_i[o0:o0 + c]
            self._master_ready = True
        prep = None
        if self.batch_sparsity:
            prep = self._prepared.pop(gb.key, None)
            if prep is None:
                prep = k.prepare(self, gb)
            k.wait_rows(prep)
        self.propagate(prep, gb)
        # the batch's user rows (final and ego) travel through the guest rows: owners fill, everybody else adds zeros
        guests = self._views.get(("guest", Bc))
        if guests is None:
            guests = self._views[("guest", Bc)] = tuple(self._guest(a, Bc) for a in (self.FIN, self.P, self.GF, self.G)) \
                                                   + (self.guest_ids[:Bc],)
        fin_g, ego_g = guests[0], guests[1]
        k.gather_rows2(fin_g, self.FIN_u, ego_g, self.P_u, gb.own_src)
        self.comm.tag = "guest_rows"
        w1 = self.comm.all_reduce_async(fin_g)
        w2 = self.comm.all_reduce_async(ego_g)
        if prep is None:
            k.fill(self.G, 0.0)
            k.fill(self.GF, 0.0)
        self.comm.wait(w1)
        self.comm.wait(w2)
        k.bpr(self.FIN, self.P, self.Ug + self.B, guests[4], gb.pos, gb.neg, self.reg_lambda, self.GF, self.G,
              self.loss, prep)
        # gradients of the guest rows go home: every owned user's occurrences are added in batch order
        k.chain_rows2(self.GF_u, guests[2], self.G_u, guests[3], gb.head_dst, gb.nxt, store=prep is not None)
        self.step_count += 1
        self.propagate_backward(prep, gb, self.step_count)
        if prep is not None:
            k.release(prep)
        return self.loss

    def prefetch(self, gb):
        """One-batch lookahead of the index-only work of the NEXT step (row bitmaps + sorted scatter plan), on
        the kernels' side stream while this step's products run."""
        if self.batch_sparsity:
            while len(self._prepared) >= 2:  # lookaheads nobody came for (a skipped batch)
                self.k.release(self._prepared.pop(next(iter(self._prepared))))
            self._prepared[gb.key] = self.k.prepare(self, gb)

    def replicated_bytes_per_step(self):
        """Bytes of per-step work every rank carries whatever the world size (what caps the speed-up): the [I] flag
        vector of the touched-item agreement, the guest rows, the batch's item rows and the loss — O(I + B d), no
        O(I d) term.  (Round 2: 12 passes over the replicated [I, d] panel = 61 GB at configs[4].)"""
        flags = 2 * 4 * self.I if (self.world > 1 and self.K >= 2 and self.I * self.d * 4 >= self.live_rows_min_bytes) else 0
        return flags + 4 * self.d * (4 * self.B + 6 * 2 * self.B)

    # ---- evaluation: users by owner, items replicated, metric sums exchanged
    def evaluate(self, test_users, test_items, excl_indptr, excl_items, top_k, reduce_sums):
        """batch_test.Test (utility/utility_train/batch_test.py:37-93) for this rank's users.
        test_users: global ids of this rank's test users (ascending), test_items: their held-out item lists;
        excl_indptr / excl_items: train CSR of THIS rank's users (local ids); reduce_sums(np.float64 array) -> the
        element-wise sum over ranks.  Returns the reference's result dict, identical on every rank."""
        import utility.utility_function.metrics as metrics

        self.propagate(None)
        local = np.asarray(test_users, dtype=np.int64) - self.lo
        kmax = max(top_k)
        sums = np.zeros(3 * len(top_k) + 1, dtype=np.float64)
        if len(local):
            top = self.k.topk(self._u(self.FIN), self.item_rows(self.FIN), local, kmax, excl_indptr, excl_items)
            r = metrics.get_label(test_items, top)
            for j, kk in enumerate(top_k):
                sums[3 * j + 0] = metrics.recall_at_k(r, kk, test_items)
                sums[3 * j + 1] = metrics.precision_at_k(r, kk, test_items)
                sums[3 * j + 2] = metrics.ndcg_at_k(r, kk, test_items)
            sums[-1] = len(local)
        sums = reduce_sums(sums)
        n_users = float(sums[-1])
        return {"recall": sums[0:-1:3] / n_users, "precision": sums[1:-1:3] / n_users, "ndcg": sums[2:-1:3] / n_users,
                "hit": np.zeros(len(top_k))}
