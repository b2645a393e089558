"""The instruments of the sharded step: the per-collective timeline and the host issue order of instrumented steps."""


# --------------------------------------------------------------------------- per-collective timeline (instrumented steps)
XGMI_PEAK_GBS = 7 * 153.0  # what one MI355X can send to its seven peers at once (MI355X_MICROARCH.md: 7 links x ~153 GB/s)


class StepTimeline:
    """What a sub-6x multi-GPU line is diagnosed from: for a few INSTRUMENTED steps after the timed
    region, per collective tag (ShardedEngine sets comm.tag before every collective): how long the collective itself
    took on the stream it ran on, how long the step's stream stalled in wait() for it, its bytes and achieved bus
    bandwidth; the host synchronisation of the touched-item agreement (if any); the step's GPU time.  HIP events only:
    the instrumented steps are slower than the timed ones by the events' own cost (~5 us each) and are never timed as
    the headline."""

    def __init__(self, torch, world):
        self.torch, self.world = torch, int(world)
        self.records = []      # (tag, kind, bytes, ev_start, ev_end) — the collective on its stream
        self.stalls = []       # (tag, ev_before_wait, ev_after_wait) on the step's stream
        self.host_syncs = []   # seconds the host spent blocked in the touched-item read-back
        self.steps = []        # (ev_begin, ev_end) per instrumented step

    def event(self):
        return self.torch.cuda.Event(enable_timing=True)

    def host_sync_begin(self):
        import time

        return time.perf_counter()

    def host_sync_end(self, t0):
        import time

        self.host_syncs.append(time.perf_counter() - t0)

    def summary(self):
        """Per-step milliseconds (averages over the instrumented steps); call after torch.cuda.synchronize()."""
        n = max(len(self.steps), 1)
        per = {}
        for tag, kind, nbytes, e0, e1 in self.records:
            r = per.setdefault(tag, {"kind": kind, "calls": 0, "bytes": 0, "collective_ms": 0.0, "stall_ms": 0.0})
            r["calls"] += 1
            r["bytes"] += nbytes
            r["collective_ms"] += e0.elapsed_time(e1)
        for tag, e0, e1 in self.stalls:
            r = per.setdefault(tag, {"kind": "?", "calls": 0, "bytes": 0, "collective_ms": 0.0, "stall_ms": 0.0})
            r["stall_ms"] += e0.elapsed_time(e1)
        bus = 2.0 * (self.world - 1) / self.world if self.world > 1 else 0.0
        out = {}
        for tag, r in per.items():
            ms = r["collective_ms"] / n
            factor = bus if r["kind"] == "all_reduce" else bus / 2.0  # reduce-scatter / all-gather: (N-1)/N of the buffer
            gbs = (r["bytes"] / n * factor / (ms * 1e-3) / 1e9) if ms > 0 else None
            out[tag] = {"kind": r["kind"], "calls_per_step": r["calls"] / n, "bytes_per_step": r["bytes"] / n,
                        "collective_ms": ms, "main_stream_stall_ms": r["stall_ms"] / n, "bus_gbs": gbs,
                        # against what one GPU can send: 7 xGMI links x 153 GB/s (MI355X_MICROARCH.md); the 8-GPU
                        # projection of DESIGN.md §7 needs >= 0.75 of it on the three panel-sized exchanges
                        "bus_frac_of_xgmi_peak": (gbs / XGMI_PEAK_GBS) if gbs is not None else None}
        step_ms = sum(a.elapsed_time(b) for a, b in self.steps) / n
        stall = sum(v["main_stream_stall_ms"] for v in out.values())
        return {"instrumented_steps": len(self.steps), "step_gpu_ms": step_ms, "main_stream_stall_ms": stall,
                "xgmi_peak_gbs": XGMI_PEAK_GBS,
                "compute_ms": step_ms - stall,
                "host_sync_ms": (sum(self.host_syncs) / n * 1e3) if self.host_syncs else 0.0,
                "collectives": out,
                "what": "per training step, averaged over the instrumented steps (run after the timed region, HIP events "
                        "around every collective and every wait): collective_ms = the collective on the stream it ran on "
                        "(for collectives enqueued on the step's own stream that time is also a stall of the step); "
                        "main_stream_stall_ms = the step's stream blocked in wait(); compute_ms = step_gpu_ms - stalls; "
                        "bus_gbs = bytes x 2(N-1)/N (all-reduce) or (N-1)/N (reduce-scatter, all-gather) / collective_ms"}


class IssueOrder:
    """The ORDER in which one rank's host enqueues a step's products and collectives — DESIGN.md §7's overlap model as a
    checked property: the projection for 8 GPUs assumes that each slice's collective is issued before the
    next slice's product, that a panel exchange is only waited for after later products have been launched, and that the
    end-of-step all-gather of the updated item rows is still in flight under the NEXT step's first item-side products.
    None of this needs hardware: it is a property of the launch sequence, so the world-8 CPU tests and the
    8-ranks-on-one-GPU rehearsal assert it, and the first real 8-GPU run can then only disappoint on link rate.

        order = IssueOrder(); order.attach(engine)      # wraps engine.comm and engine.k
        order.begin_step(); engine.train_step(gb); ...
        assert not order.violations()

    events: ("step", i) | ("product", "user") | ("product", "item", j) | ("issue", tag, j) | ("wait", tag, j)."""

    SLICED = ("panel", "reduce_scatter")  # tags of collectives issued slice by slice from _item_side

    def __init__(self):
        self.events, self.n_steps, self.n_slices = [], 0, 1
        self.packed_violations = None

    def attach(self, eng):
        self.n_slices = len(eng.slices)
        # the 24-bit panel exchange keeps its own record of the order of its halves (Packed24Comm.order_violations):
        # slice j + 1's all-to-all queued before slice j's sum and all-gather
        self.packed_violations = getattr(eng.comm, "order_violations", None)
        names = {id(eng.G_ui): ("user",)}
        names.update({id(sl[0]): ("item", j) for j, sl in enumerate(eng.slices)})
        if isinstance(eng.comm, TimelineComm):
            eng.comm.order = self
        else:
            eng.comm = OrderComm(eng.comm, self)
        eng.k = OrderKernels(eng.k, self, names)
        return self

    def begin_step(self):
        self.events.append(("step", self.n_steps))
        self.n_steps += 1

    def end_steps(self):
        """What follows (the caller draining the last all-gather, evaluation) is not part of a step."""
        self.events.append(("end",))

    def steps(self):
        out, live = [], False
        for e in self.events:
            if e[0] == "step":
                out.append([])
                live = True
            elif e[0] == "end":
                live = False
            elif live:
                out[-1].append(e)
        return out

    def violations(self):
        """Every way the recorded sequence departs from the overlap model, as strings (empty list = as designed)."""
        bad, S = [], self.n_slices
        steps = self.steps()
        for si, ev in enumerate(steps):
            tags = []
            for i, e in enumerate(ev):
                if e[0] == "issue" and e[2] is not None and e[1].endswith(self.SLICED):
                    if e[1] not in tags:
                        tags.append(e[1])
                    # (1) a slice's collective goes out right behind that slice's product, before the next slice's
                    if i == 0 or ev[i - 1] != ("product", "item", e[2]):
                        bad.append("step %d: %s slice %d issued after %r, not right behind its own product" % (si, e[1], e[2], ev[i - 1] if i else None))
            for tag in tags:
                issued = [i for i, e in enumerate(ev) if e[0] == "issue" and e[1] == tag]
                waits = [i for i, e in enumerate(ev) if e[0] == "wait" and e[1] == tag]
                if len(issued) != S:
                    bad.append("step %d: %s issued for %d slices of %d" % (si, tag, len(issued), S))
                if not waits:
                    bad.append("step %d: %s never waited for inside the step" % (si, tag))
                    continue
                # (2) nobody waits for a sliced exchange before later products have been launched behind its last slice
                if not any(e[0] == "product" for e in ev[issued[-1] + 1: waits[0]]):
                    bad.append("step %d: %s waited for with no product launched behind it" % (si, tag))
            # (3) the updated item rows go round slice by slice: slice j's all-gather is out before slice j + 1's
            #     reduce-scatter is waited for
            ag = {e[2]: i for i, e in enumerate(ev) if e[0] == "issue" and e[1] == "item_table.all_gather"}
            rs = {e[2]: i for i, e in enumerate(ev) if e[0] == "wait" and e[1].endswith("reduce_scatter")}
            if len(ag) != S:
                bad.append("step %d: %d all-gathers of the updated item rows for %d slices" % (si, len(ag), S))
            for j in range(S - 1):
                if j in ag and j + 1 in rs and not ag[j] < rs[j + 1]:
                    bad.append("step %d: all-gather of slice %d issued after the wait for slice %d's reduce-scatter" % (si, j, j + 1))
            if any(e[0] == "wait" and e[1] == "item_table.all_gather" for e in ev[(ag[0] if 0 in ag else len(ev)):]):
                bad.append("step %d: the end-of-step all-gather is waited for inside its own step" % si)
            # (4) ... and is still in flight under the next step's first item-side products (which read local user rows only)
            if si > 0:
                w = [i for i, e in enumerate(ev) if e[0] == "wait" and e[1] == "item_table.all_gather"]
                first_user = next((i for i, e in enumerate(ev) if e == ("product", "user")), len(ev))
                n_before = sum(1 for e in ev[: (w[0] if w else 0)] if e[0] == "product" and e[1] == "item")
                if len(w) != S:
                    bad.append("step %d: %d waits for the previous step's %d all-gathers" % (si, len(w), S))
                elif n_before < S:
                    bad.append("step %d: the previous step's all-gather is waited for after %d of %d first-layer item-side "
                               "products" % (si, n_before, S))
                elif w[-1] > first_user:
                    bad.append("step %d: a user-side product (reads the item table) launched before the table was whole" % si)
        if self.packed_violations is not None:
            bad += ["24-bit exchange: " + v for v in self.packed_violations()]
        return bad

    def summary(self):
        return {"steps": self.n_steps, "slices": self.n_slices, "events": len(self.events), "violations": self.violations(),
                "what": "host issue order of the instrumented steps' products and collectives on this rank, checked against "
                        "DESIGN.md §7's overlap model (IssueOrder.violations): slice j's collective right behind slice j's "
                        "product; sliced exchanges waited for only after later products were launched; the end-of-step "
                        "all-gather waited for in the NEXT step, behind its first-layer item-side products"}


class OrderComm:
    """A comm wrapper that only records issue / wait order (IssueOrder); no events, no timing: CPU tests use it."""

    def __init__(self, inner, order):
        self.inner, self.order = inner, order
        self.world, self.rank = inner.world, inner.rank
        self.averages = getattr(inner, "averages", False)
        self.tag, self.slice = "untagged", None

    def all_reduce_async(self, t, average=False):
        self.order.events.append(("issue", self.tag, self.slice))
        return (self.inner.all_reduce_async(t, average), self.tag, self.slice)

    def all_gather_async(self, out, t):
        self.order.events.append(("issue", self.tag, self.slice))
        return (self.inner.all_gather_async(out, t), self.tag, self.slice)

    def reduce_scatter_async(self, t):
        self.order.events.append(("issue", self.tag, self.slice))
        return (self.inner.reduce_scatter_async(t), self.tag, self.slice)

    def wait(self, handle):
        if handle is None:
            return
        work, tag, sl = handle
        self.order.events.append(("wait", tag, sl))
        self.inner.wait(work)

    def __getattr__(self, name):
        return getattr(self.inner, name)


class OrderKernels:
    """A `kernels` wrapper that records every product launch (which operator: the user-side block or item slice j)."""

    def __init__(self, inner, order, names):
        self._inner, self._order, self._names = inner, order, names

    def spmm(self, graph, X, **kw):
        self._order.events.append(("product",) + self._names.get(id(graph), ("other",)))
        return self._inner.spmm(graph, X, **kw)

    def __getattr__(self, name):
        return getattr(self._inner, name)


class TimelineComm:
    """Wraps a comm (NativeComm / TorchComm / test comms) and fills a StepTimeline.  The collective's own duration is
    measured on the stream it runs on when the inner comm says which (NativeComm.timed_stream); otherwise between two
    events on the step's stream around the call (exact for collectives enqueued there, a lower bound — the issue cost —
    for a process group's internal stream, whose end is then taken at the matching wait())."""

    def __init__(self, inner, timeline):
        self.inner, self.tl = inner, timeline
        self.world, self.rank = inner.world, inner.rank
        self.averages = getattr(inner, "averages", False)
        self.tag, self.slice = "untagged", None
        self.order = None  # an IssueOrder: the same instrumented steps also record their issue order

    def _issue(self, kind, nbytes, call):
        torch, tl = self.tl.torch, self.tl
        if self.order is not None:
            self.order.events.append(("issue", self.tag, self.slice))
        e0, e1 = tl.event(), tl.event()
        own = getattr(self.inner, "timed_stream", None)
        stream = own(nbytes) if own is not None else None  # the torch stream the inner comm will run this one on
        if stream is None:
            e0.record()
            work = call()
            e1.record()
            rec = [self.tag, kind, nbytes, e0, e1]
            self.tl.records.append(rec)
            return (work, rec if work is not None else None, self.tag, self.slice)
        issued = torch.cuda.Event()
        issued.record()
        stream.wait_event(issued)   # (what the inner comm does next: the start event sits behind the same dependency)
        e0.record(stream)
        work = call()
        e1.record(stream)
        self.tl.records.append([self.tag, kind, nbytes, e0, e1])
        return (work, None, self.tag, self.slice)

    def _bytes(self, numel):
        # (a packed exchange puts 3 bytes per value on the wire: Packed24Comm.wire_bytes)
        f = getattr(self.inner, "wire_bytes", None)
        return f(numel) if f is not None else numel * 4

    def all_reduce_async(self, t, average=False):
        return self._issue("all_reduce", self._bytes(t.numel()), lambda: self.inner.all_reduce_async(t, average))

    def all_gather_async(self, out, t):
        return self._issue("all_gather", self._bytes(out.numel()), lambda: self.inner.all_gather_async(out, t))

    def reduce_scatter_async(self, t):
        return self._issue("reduce_scatter", self._bytes(t.numel()), lambda: self.inner.reduce_scatter_async(t))

    def wait(self, handle):
        if handle is None:
            return
        work, rec, tag, sl = handle
        if self.order is not None:
            self.order.events.append(("wait", tag, sl))
        a, b = self.tl.event(), self.tl.event()
        a.record()
        self.inner.wait(work)
        b.record()
        self.tl.stalls.append((tag, a, b))
        if rec is not None:
            rec[4] = b  # a work object's collective ends (at the latest) where its wait() returns on the step's stream

    def __getattr__(self, name):
        return getattr(self.inner, name)
