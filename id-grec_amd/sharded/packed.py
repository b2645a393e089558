"""The explicit panel exchange of the sharded step: 24-bit rows or fp32 blocks, summed in rank order (opt-in)."""
import numpy as np


# --------------------------------------------------------------------------- the panel exchanges as 24-bit rows (opt-in)
class Packed24Comm:
    """A comm wrapper (around NativeComm / TorchComm / NoComm / the tests' comms): the step's LARGE exchanges — the two
    [I, d] all-reduces, the reduce-scatter of the last backward product, the all-gather of the updated item rows, the
    touched-item row sets — travel as 24-bit values (idg_pack24_f32: sign, exponent, 15 mantissa bits, rounded to nearest;
    2^-16 = 1.5e-5 relative, inside the north star's 1e-4) and are summed by this library's own kernel IN RANK ORDER:

        all-reduce      pack -> all-to-all (block p to rank p) -> reduce24 (q0 + q1 + ... in rank order, packed again)
                        -> all-gather of the packed sums -> unpack (EVERY rank, the owner included, holds the same bits)
        reduce-scatter  pack -> all-to-all -> reduce24 into the own fp32 block
        all-gather      pack the own block -> all-gather -> unpack (the own block too: replicas stay bit-identical)

    3/4 of the fp32 exchange's bytes on the links (what lowers the link rate >= 6x at 8 GPUs needs from 88 %
    to 66 % of the xGMI peak), and a k-GPU run is bit-reproducible run to run whatever algorithm RCCL would pick
    (SURVEY.md 8e).  Collectives below `min_bytes` (the batch's guest rows, whose exchange must stay exact: x + 0 + ...)
    or whose length does not divide by 4 x world stay with the inner comm, in fp32.

    Streams (kernels.exchange_stream): pack runs on the step's stream right behind the product; the all-to-all is issued
    from there; the second half — wait for the all-to-all, reduce24, all-gather, unpack — runs on the exchange's own
    stream, and is issued only AFTER the next slice's first half (slice j + 1's all-to-all is queued before slice j's
    all-gather, so the links are not idle while slice j is being summed).  wait() joins the step's stream.
    `log` records the order of the halves (IssueOrder checks it); `stats()` the bytes put on the wire."""

    averages = False
    by_blocks = True   # (the engine hands over slices that divide into one block per rank: the padded views)

    def __init__(self, inner, kernels, min_bytes=4 << 20, bits=24):
        """bits = 32: the same explicit exchange on fp32 values — no packing, RCCL's bytes on the links, the rank-ordered sum
        (idg_reduce_blocks_f32): reproducible without the 2^-16 quantisation (`bench.py --reduce-order rank`)."""
        assert bits in (24, 32)
        self.inner, self.k = inner, kernels
        self.world, self.rank = int(inner.world), int(inner.rank)
        self.bits, self.packed = int(bits), bits == 24
        self.min_bytes = int(min_bytes)
        self._free = {}        # words -> [(snd, rcv), ...] buffers not in flight
        self._pending = []     # exchanges whose second half has not been issued yet, oldest first
        self._seq = 0
        self.log = []          # ("first" | "second" | "wait", seq, kind)
        self._pre = {}         # (address, length) of a tensor -> (snd, rcv) its producer is writing packed values into
        self.wire = {"packed_bytes_sent": 0, "fp32_bytes_it_replaces": 0, "exchanges": 0, "fp32_collectives": 0,
                     "packed_by_producer": 0}

    # ---- helpers
    @staticmethod
    def _n(t):
        return int(t.size) if isinstance(t, np.ndarray) else int(t.numel())

    @staticmethod
    def _flat(t):
        return t.reshape(-1)

    def _eligible(self, n):
        return n * 4 >= self.min_bytes and n % (4 * self.world) == 0

    def _buffers(self, words):
        """(send, receive) buffers of `words` 32-bit words: views of buffers kept per SIZE CLASS (the next power of two —
        the touched-item exchanges come in a different length for nearly every batch: one pool entry per length would
        grow without bound over a training run)."""
        cls = 1 << max(int(words) - 1, 0).bit_length()
        pool = self._free.setdefault(cls, [])
        # (fp32 blocks: the tensor itself is the send buffer — only the receive side needs one)
        snd, rcv = pool.pop() if pool else (self.k.zeros((cls if self.packed else 1,)), self.k.zeros((cls,)))
        return snd[:words], rcv[:words], (cls, snd, rcv)

    def _words(self, n):
        return n // 4 * 3 if self.packed else n

    def _count(self, n_values, phases):
        # a rank sends (N - 1) / N of the buffer in each phase (all-to-all, all-gather)
        share = (self.world - 1) / self.world
        self.wire["packed_bytes_sent"] += int(phases * share * n_values * (3 if self.packed else 4))
        self.wire["fp32_bytes_it_replaces"] += int(phases * share * n_values * 4)
        self.wire["exchanges"] += 1

    class _X:
        __slots__ = ("seq", "kind", "t", "n", "snd", "rcv", "home", "work", "done", "second", "own")

    def _first_half(self, kind, t, n):
        """pack + all-to-all of t's n values (kind "ar" / "rs"), on the current (the step's) stream."""
        words = self._words(n)
        x = self._X()
        x.seq, x.kind, x.t, x.n, x.second, x.done, x.own = self._seq, kind, t, n, False, None, None
        self._seq += 1
        pre = self._pre.pop(self._key(t), None)
        if pre is not None:   # the producer has written the packed values itself (packed_target)
            x.snd, x.rcv, x.home = pre
            self.wire["packed_by_producer"] += 1
        elif self.packed:
            x.snd, x.rcv, x.home = self._buffers(words)
            self.k.pack24(self._flat(t), x.snd, n)
        else:                 # fp32 blocks: the tensor itself is the send buffer
            _, x.rcv, x.home = self._buffers(words)
            x.snd = self._flat(t)
        x.work = self.inner.all_to_all_async(x.rcv, x.snd)
        self.log.append(("first", x.seq, kind))
        # the exchange before this one may now go on: its sum and its all-gather queue BEHIND this all-to-all
        self._flush(keep=x)
        self._pending.append(x)
        return x

    def _second_half(self, x):
        k, N = self.k, self.world
        blk_words, blk_n = self._words(x.n) // N, x.n // N
        with k.exchange_stream():
            self.inner.wait(x.work)
            if not self.packed:
                own = x.snd[self.rank * blk_n:(self.rank + 1) * blk_n]   # (x.snd is the tensor itself)
                k.reduce_blocks(x.rcv, N, blk_n, own)
                if x.kind == "ar":
                    self.inner.wait(self.inner.all_gather_async(x.snd, own))
            elif x.kind == "rs":
                own = self._flat(x.t)[self.rank * blk_n:(self.rank + 1) * blk_n]
                k.reduce24(x.rcv, N, blk_n, out_f32=own)
            else:
                own = x.snd[self.rank * blk_words:(self.rank + 1) * blk_words]
                k.reduce24(x.rcv, N, blk_n, out_packed=own)
                self.inner.wait(self.inner.all_gather_async(x.snd, own))
                k.unpack24(x.snd, self._flat(x.t), x.n)
            x.done = k.record_event()
        x.second = True
        self.log.append(("second", x.seq, x.kind))

    def _flush(self, keep=None):
        while self._pending and self._pending[0] is not keep:
            self._second_half(self._pending.pop(0))

    @staticmethod
    def _key(t):
        return (t.ctypes.data, t.size) if isinstance(t, np.ndarray) else (t.data_ptr(), t.numel())

    def packed_target(self, t, n_valid=None):
        """The send buffer of the NEXT all_reduce_async / reduce_scatter_async of `t`, for a producer that writes its result
        packed by itself (the item-side product's y24 epilogue: no fp32 write of the partial, no pack pass) — or None when
        that collective would not travel packed.  n_valid: the values the producer will write (the rest of t is zero:
        a slice's padding rows)."""
        n = self._n(t)
        if not self.packed or not self._eligible(n):
            return None
        snd, rcv, home = self._buffers(n // 4 * 3)
        if n_valid is not None and n_valid < n:
            snd[n_valid // 4 * 3:] = 0
        old = self._pre.pop(self._key(t), None)
        if old is not None:  # (a target nobody came for: its buffers go back)
            self._free[old[2][0]].append(old[2][1:])
        self._pre[self._key(t)] = (snd, rcv, home)
        return snd

    # ---- the comm interface
    def all_reduce_async(self, t, average=False):
        n = self._n(t)
        if not self._eligible(n):
            self.wire["fp32_collectives"] += 1
            return ("inner", self.inner.all_reduce_async(t, average))
        assert not average, "Packed24Comm sums"
        self._count(n, 2)
        return ("packed", self._first_half("ar", t, n))

    def reduce_scatter_async(self, t):
        n = self._n(t)
        if not self._eligible(n):
            self.wire["fp32_collectives"] += 1
            return ("inner", self.inner.reduce_scatter_async(t))
        self._count(n, 1)
        return ("packed", self._first_half("rs", t, n))

    def all_gather_async(self, out, t):
        n, nb = self._n(out), self._n(t)
        if not self.packed or not self._eligible(n) or nb * self.world != n:
            self.wire["fp32_collectives"] += 1
            if self._pending:
                self._flush()  # (collectives go out in program order on every rank)
            return ("inner", self.inner.all_gather_async(out, t))
        self._count(n, 1)
        self._flush()  # (an all-gather has no first half to hide a sum behind: whatever is pending goes first)
        words, blk_words = n // 4 * 3, nb // 4 * 3
        x = self._X()
        x.seq, x.kind, x.t, x.n, x.second = self._seq, "ag", out, n, True
        self._seq += 1
        x.snd, x.rcv, x.home = self._buffers(words)
        own = x.snd[self.rank * blk_words:(self.rank + 1) * blk_words]
        self.k.pack24(self._flat(t), own, nb)
        x.work = self.inner.all_gather_async(x.snd, own)
        self.log.append(("first", x.seq, "ag"))
        with self.k.exchange_stream():
            self.inner.wait(x.work)
            self.k.unpack24(x.snd, self._flat(out), n)
            x.done = self.k.record_event()
        self.log.append(("second", x.seq, "ag"))
        return ("packed", x)

    def all_to_all_async(self, recv, send):
        return ("inner", self.inner.all_to_all_async(recv, send))

    def wire_bytes(self, numel):
        """Bytes a collective over `numel` values moves per unit of buffer (TimelineComm's bus-rate arithmetic)."""
        return numel * (3 if (self.packed and self._eligible(numel)) else 4)

    def timed_stream(self, nbytes):
        return None  # (a compound exchange: TimelineComm brackets it on the step's stream, issue to wait)

    def wait(self, handle):
        if handle is None:
            return
        kind, x = handle
        if kind == "inner":
            self.inner.wait(x)
            return
        if not x.second:  # nobody issued a later exchange behind it: its second half goes out now (and all before it)
            while self._pending:
                y = self._pending.pop(0)
                self._second_half(y)
                if y is x:
                    break
        self.k.wait_event(x.done)
        self.log.append(("wait", x.seq, x.kind))
        self._free[x.home[0]].append(x.home[1:])
        x.snd = x.rcv = x.t = x.home = None

    def __getattr__(self, name):
        return getattr(self.inner, name)

    # ---- evidence
    def order_violations(self):
        """The halves' issue order against the pipeline this class promises: every first half is followed by its second
        half exactly once and waited for after it; the second half of exchange i is never issued before the first half
        of exchange i + 1 when that one was issued before i was waited for (its all-to-all is in the queue first)."""
        bad, pos = [], {}
        for i, (what, seq, kind) in enumerate(self.log):
            pos.setdefault(seq, {})[what] = i
        for seq, p in sorted(pos.items()):
            if "first" in p and "second" not in p and "wait" in p:
                bad.append("exchange %d waited for without its second half" % seq)
            if "second" in p and "first" in p and not p["first"] < p["second"]:
                bad.append("exchange %d: second half before the first" % seq)
            if "wait" in p and "second" in p and not p["second"] < p["wait"]:
                bad.append("exchange %d: waited for before its second half was issued" % seq)
            nxt = pos.get(seq + 1)
            # (an all-gather has no all-to-all to queue ahead: it flushes what is pending and is not part of this rule)
            if nxt and "first" in nxt and "wait" in p and nxt["first"] < p["wait"] and p.get("second", 0) < nxt["first"] \
                    and self.log[p["first"]][2] != "ag" and self.log[nxt["first"]][2] != "ag":
                bad.append("exchange %d: its sum / all-gather was issued before exchange %d's all-to-all (no overlap)" % (seq, seq + 1))
        return bad

    def release_buffers(self):
        """Drop the pooled send / receive buffers (nothing may be in flight): the bench frees them before rank 0 builds the
        single-GPU reference."""
        assert not self._pending, "an exchange is still in flight"
        self._free.clear()
        self._pre.clear()

    def stats(self):
        w = dict(self.wire)
        w["ratio"] = (w["packed_bytes_sent"] / w["fp32_bytes_it_replaces"]) if w["fp32_bytes_it_replaces"] else None
        w["order_violations"] = self.order_violations()
        return w


RankOrderComm = Packed24Comm  # (bits = 32: the explicit exchange and the rank-ordered sum on fp32 values)
