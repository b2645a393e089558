"""The sharded step at world size 1 on a fixed small graph (1000 users x 640 items, ~30000 edges from synth; d = 64, K = 3,
B = 256, two item slices, six train_steps with prefetch, two seeds) through three communicators: NoComm, the explicit
exchange on 24-bit rows and on fp32 blocks (Packed24Comm around NoComm, min_bytes = 0), and the same two around a NoComm
that returns events (EventNoComm below: the runs whose bits are reproducible).  Prints a checksum of the raw bits
of the tables and of the loss per run, the explicit exchanges' own order check, and — after one further step instrumented
as the bench driver does it (TimelineComm + IssueOrder) — the issue-order violations and the timeline's keys.
Uses the public names of idgrec_amd.sharded only: copy it into another revision's tree (it imports the tree it lies in),
run both with the same library (IDG_LIB_PATH); equal lines = the two trees launch and compute the same."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

import idgrec_amd.sharded as sh
import idgrec_amd.synth as S

U, I, E, d, K, B, STEPS = 1000, 640, 30000, 64, 3, 256, 6
users, items = S.generate(U, I, E, seed=0)
deg = np.bincount(users, minlength=U)
ui, iu = sh.shard_adjacency_from_edges(users, items, U, I, 0, U)


def digest(t):
    return hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest()[:12]


class EventNoComm(sh.NoComm):
    """NoComm whose all-to-all and all-gather hand back an event on the stream they ran on, as NativeComm's second-stream
    route does.  Over plain NoComm (handle None, wait() a no-op) nothing orders Packed24Comm's second half, on the
    exchange's own stream, behind the first half on the step's stream (the cross-stream finding): those runs'
    checksums may differ from run to run of ONE tree.  Over this comm they may not."""

    def all_to_all_async(self, recv, send):
        super().all_to_all_async(recv, send)
        return kern.record_event()

    def all_gather_async(self, out, t):
        super().all_gather_async(out, t)
        return kern.record_event()

    def wait(self, work):
        kern.wait_event(work)


def comms(kern):
    yield "NoComm", sh.NoComm()
    yield "Packed24Comm bits=24", sh.Packed24Comm(sh.NoComm(), kern, min_bytes=0, bits=24)
    yield "Packed24Comm bits=32", sh.Packed24Comm(sh.NoComm(), kern, min_bytes=0, bits=32)
    yield "ordered      bits=24", sh.Packed24Comm(EventNoComm(), kern, min_bytes=0, bits=24)
    yield "ordered      bits=32", sh.Packed24Comm(EventNoComm(), kern, min_bytes=0, bits=32)


for seed in (0, 1):
    tri = S.draw_triples(seed, users, items, U, I, (STEPS + 1) * B)[0]
    g = torch.Generator().manual_seed(seed)
    W_u = (torch.rand(U, d, generator=g) * 2 - 1) * (6.0 / (U + d)) ** 0.5
    W_i = (torch.rand(I, d, generator=g) * 2 - 1) * (6.0 / (I + d)) ** 0.5
    kern = sh.HipKernels()
    for name, comm in comms(kern):
        eng = sh.ShardedEngine(kern, comm, ui, iu, U, I, d, K, True, 1e-4, 1e-3, batch_size=B, user_lo=0, n_slices=2,
                               live_rows_min_bytes=0, global_user_degree=deg)
        assert len(eng.slices) == 2
        eng.P[:U].copy_(W_u)
        eng.item_rows(eng.P).copy_(W_i)
        batches = [eng.make_batch(*(tri[s * B:(s + 1) * B, c] for c in range(3))) for s in range(STEPS + 1)]
        for s in range(STEPS):
            eng.prefetch(batches[s + 1])
            eng.train_step(batches[s])
        eng._wait_item_table()
        torch.cuda.synchronize()
        print("seed %d  %-21s P %s  loss %s" % (seed, name, digest(eng.P), digest(eng.loss)), flush=True)
        if name != "NoComm":
            print("seed %d  %-21s order_violations %r" % (seed, name, comm.order_violations()), flush=True)
        # one further step, instrumented as run_sharded_bench instruments its last ones
        tl = sh.StepTimeline(torch, 1)
        eng.comm, eng.timeline = sh.TimelineComm(eng.comm, tl), tl
        order = sh.IssueOrder().attach(eng)
        ev = (tl.event(), tl.event())
        ev[0].record()
        order.begin_step()
        eng.train_step(batches[STEPS])
        ev[1].record()
        tl.steps.append(ev)
        order.end_steps()
        eng._wait_item_table()
        torch.cuda.synchronize()
        summary = tl.summary()
        print("seed %d  %-21s instrumented step: P %s  loss %s  issue order %r" % (seed, name, digest(eng.P), digest(eng.loss), order.violations()), flush=True)
        print("seed %d  %-21s timeline keys %s  collectives %s" % (seed, name, sorted(summary), sorted(summary["collectives"])), flush=True)
        del eng, batches
    kern.close()
