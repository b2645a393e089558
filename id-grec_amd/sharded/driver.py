"""`bench.py --gpus N`: the sharded bench driver with its parity capture and compare."""
import os

import numpy as np

from .instruments import IssueOrder, StepTimeline, TimelineComm
from .kernels import HipKernels
from .packed import Packed24Comm
from .partition import partition_users_by_nnz, shard_adjacency_from_edges
from .step import ShardedEngine


# --------------------------------------------------------------------------- bench driver
PARITY_TOL = 1e-4  # BASELINE.json north_star: "within 1e-4 relative on fp32 embeddings and loss"


def parity_capture(eng, batches, tri, dist, rank, lo, hi, num_users, num_items, seed=0, n_sample=1024):
    """The N-rank half of `parity_vs_1gpu` (the only place RCCL between devices ever runs — the driver's
    `bench.py --gpus N` — must carry its own correctness evidence).  Runs the steps `batches` (GlobalBatch list; `tri` their
    global triples [n * B, 3]) on the freshly initialised sharded engine — every rank calls this — and returns on rank 0
    what the single-device engine has to reproduce from the same tables and batches (the oracle of a k-GPU
    run is the 1-GPU result):
      loss [n, 2]; per step FIN at the batch's user rows (the guest rows: batch order) and at its distinct item rows;
      after the last step, table rows of a sample of users (each from its owner, summed over the ranks: x + 0 + ...) and
      items (replicated): the batch's own and `n_sample` random ones of each side.
    Leaves the engine n steps into training (the timed region goes on from there)."""
    import torch

    B = eng.B
    n = len(batches)
    host = dist.get_backend() != "nccl"
    rng = np.random.default_rng(seed + 12345)
    user_ids = np.unique(np.concatenate([tri[:, 0], rng.integers(0, num_users, n_sample)])).astype(np.int64)
    item_ids = np.unique(np.concatenate([tri[:, 1], tri[:, 2], rng.integers(0, num_items, n_sample)])).astype(np.int64)

    def user_rows():
        mine = (user_ids >= lo) & (user_ids < hi)
        buf = torch.zeros((len(user_ids), eng.d), dtype=torch.float32, device=eng.P.device)
        if mine.any():
            buf[torch.from_numpy(np.nonzero(mine)[0]).to(buf.device)] = eng.P[torch.from_numpy(user_ids[mine] - lo).to(buf.device)]
        buf = buf.cpu() if host else buf
        dist.all_reduce(buf)
        return buf.cpu()

    eng._wait_item_table()
    item_dev = torch.from_numpy(item_ids).to(eng.P.device)
    out = {"triples": np.ascontiguousarray(tri), "user_ids": user_ids, "item_ids": item_ids, "user_rows_before": user_rows(),
           "item_rows_before": eng.item_rows(eng.P)[item_dev].cpu(), "loss": [], "fin_users": [], "fin_items": [],
           "fin_item_ids": []}
    for i, gb in enumerate(batches):
        eng.train_step(gb)
        if i == 0 and rank == 1 and os.environ.get("IDG_BENCH_TEST_BREAK_PARITY") == "1":
            eng._wait_item_table()
            eng.P_u.mul_(1.001)  # tests only: stands in for a broken exchange (tests/test_bench_contract.py)
        out["loss"].append(eng.loss.double().cpu().numpy().copy())
        out["fin_users"].append(eng._guest(eng.FIN, gb.B).cpu())
        out["fin_items"].append(eng.item_rows(eng.FIN)[gb.items].cpu())
        out["fin_item_ids"].append(gb.items.cpu().numpy())
    eng._wait_item_table()
    out["user_rows"] = user_rows()
    out["item_rows"] = eng.item_rows(eng.P)[item_dev].cpu()
    out["loss"] = np.stack(out["loss"])
    assert tri.shape[0] == n * B
    return out if rank == 0 else None


def parity_compare(single, captured, tol=PARITY_TOL):
    """The 1-GPU half: `single` = a freshly initialised PropagationEngine on the WHOLE graph with the same initial tables;
    runs the captured batches through it and returns the `parity_vs_1gpu` object of the bench line — relative errors
    (Frobenius norms over the compared rows; the loss: largest over steps and terms) of the N-rank run against this one,
    and `ok` = all three within tol and `update_rel_err` — the same table rows as UPDATES since the initial tables: an
    N-rank step that left the tables alone would show there — within 100 x tol."""
    import torch

    tri = torch.from_numpy(captured["triples"]).to(single.params.device)
    B = captured["fin_users"][0].shape[0]
    U = single.U
    dev = single.params.device
    urows = torch.from_numpy(captured["user_ids"]).to(dev)
    irows = torch.from_numpy(captured["item_ids"]).to(dev) + U
    before = torch.cat([single.params[urows], single.params[irows]]).cpu()
    init_n = torch.cat([captured["user_rows_before"], captured["item_rows_before"]])
    init_equal = bool(torch.equal(before, init_n))

    def rel(a, b):
        return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))

    loss_err, fin_err = 0.0, 0.0
    loss_1 = []
    for i in range(len(captured["fin_users"])):
        u, p, n = (tri[i * B:(i + 1) * B, c].contiguous() for c in range(3))
        loss = single.train_step(u, p, n).double().cpu().numpy().copy()
        loss_1.append(loss)
        loss_err = max(loss_err, float(np.max(np.abs(captured["loss"][i] - loss) / np.maximum(np.abs(loss), 1e-30))))
        items = torch.from_numpy(captured["fin_item_ids"][i]).to(dev)
        fin_1 = torch.cat([single.final[u], single.final[items + U]]).cpu()
        fin_n = torch.cat([captured["fin_users"][i], captured["fin_items"][i]])
        fin_err = max(fin_err, rel(fin_n, fin_1))
    after_1 = torch.cat([single.params[urows], single.params[irows]]).cpu()
    after_n = torch.cat([captured["user_rows"], captured["item_rows"]])
    table_err = rel(after_n, after_1)
    upd_err = rel(after_n - init_n, after_1 - before)
    # (the first steps of a run start at loss ~ ln 2 whatever the tables hold, and the tables move by ~lr per step against
    #  values of ~1e-2: the UPDATES are the sensitive quantity — a loose bound on them is part of the verdict)
    tol_update = 100 * tol
    ok = bool(init_equal and loss_err <= tol and fin_err <= tol and table_err <= tol and upd_err <= tol_update)
    return {"what": "%d training steps from the same initial tables and the same global batches on the N ranks and on ONE "
                    "device (the fused single-GPU engine, rank 0, same run): N-rank result against the 1-GPU result — loss: "
                    "largest relative error over steps and terms; final_rows: FIN at every batch's user and item rows; table: "
                    "%d sampled user + %d item rows after the last Adam step (each batch's own + random ones); relative "
                    "Frobenius norms.  SURVEY.md 8e: the oracle of a k-GPU run is the 1-GPU result"
                    % (len(loss_1), len(captured["user_ids"]), len(captured["item_ids"])),
            "steps": len(loss_1), "loss_rel_err": loss_err, "final_rows_rel_err": fin_err, "table_rel_err": table_err,
            "update_rel_err": upd_err, "table_max_abs_err": float((after_n - after_1).abs().max()),
            "initial_tables_equal": init_equal, "loss_n_ranks": [[float(x) for x in row] for row in captured["loss"]],
            "loss_1_gpu": [[float(x) for x in row] for row in loss_1], "tol": tol, "tol_update": tol_update, "ok": ok}


def run_sharded_bench(args, rank, world, dist, comm, comm_name, single_gpu_reference=None):
    """bench.py --gpus N (N > 1), the north-star split: ONE graph of the named shape cut across the
    ranks by nnz-balanced user-row blocks, item table replicated, ONE global batch of B triples per step (the
    reference takes one Adam step per batch_size triples, trainer.py:36-56) — strong scaling: value = B*steps /
    max-over-ranks time.  single_gpu_reference(args) -> dict: called on rank 0 AFTER the timed region and after the shards
    are freed, it measures the SAME workload unsharded on this rank's GPU (bench.py); the line then carries
    speedup_vs_1gpu.  Returns the bench line (rank 0) or None; the caller emits it and ends the process group."""
    import time

    import torch

    from .. import synth as S

    phase = getattr(args, "phase", None) or (lambda name: None)  # bench.py's supervisor quotes it if the run is ended
    phase("graph")
    U, I, E = S.SHAPES[args.workload]
    d, K, B = args.dim, args.layers, args.batch
    # every rank needs the same global graph: large ones are drawn once per machine, then loaded
    if world > 1 and E >= int(os.environ.get("IDG_SYNTH_SHARED_MIN_EDGES", "50000000")):
        users, items = S.generate_shared(U, I, E, 0, rank, dist.barrier)
    else:
        users, items = S.generate(U, I, E, seed=0)
    user_degree = np.bincount(users, minlength=U)
    bounds = partition_users_by_nnz(user_degree, world)
    lo, hi = int(bounds[rank]), int(bounds[rank + 1])
    ui, iu = shard_adjacency_from_edges(users, items, U, I, lo, hi)  # this rank's rows only: no global CSR
    nnz_global, n_edges = 2 * len(users), len(users)
    # slices of the item panel: what a collective moves at a time.  From 4 ranks on the communicator's stream is the
    # critical path and a collective can start when its first slice exists: finer slices there
    n_slices = int(getattr(args, "item_slices", 0) or 0) or ((8 if world >= 4 else 4) if I * d * 4 >= (256 << 20) else 1)
    cuts = partition_users_by_nnz(np.bincount(items, minlength=I), n_slices)  # same cuts on every rank: global item degrees
    n_timeline = 3 if world > 1 or os.environ.get("IDG_BENCH_TIMELINE") == "1" else 0  # instrumented steps, after the timed ones
    # parity_vs_1gpu: the first n_parity batches run BEFORE the warm-up, on the fresh tables, and rank 0's single-GPU
    # reference repeats them after the timed region (no reference in this run -> nothing to compare with)
    n_parity = max(int(getattr(args, "parity_steps", 3)), 0) if single_gpu_reference is not None else 0
    need = (n_parity + args.steps + args.warmup + n_timeline) * B
    tri = S.draw_triples(args.seed, users, items, U, I, need)[0]  # the same global sequence on every rank
    edges = (users, items) if (rank == 0 and single_gpu_reference is not None) else None  # (rank 0 measures the 1-GPU point later)
    del users, items
    phase("engine")
    kern = HipKernels()
    panel_bits = int(getattr(args, "panel_bits", 32) or 32)
    rank_order = panel_bits == 24 or getattr(args, "reduce_order", "rccl") == "rank"
    if rank_order:
        # opt-in: the panel-sized exchanges as an explicit exchange summed in rank order by this library's own kernel —
        # 24-bit rows (idg_reduce24_f32) or fp32 blocks (idg_reduce_blocks_f32)
        comm = Packed24Comm(comm, kern, bits=panel_bits)
        comm_name += (" + 24-bit panel exchange (pack -> all-to-all -> rank-ordered sum -> all-gather)" if panel_bits == 24 else
                      " + explicit fp32 panel exchange (all-to-all -> rank-ordered sum -> all-gather)")
    # global_user_degree: the touched-item exchanges are sized by a host-side bound — no host synchronisation in the step
    eng = ShardedEngine(kern, comm, ui, iu, hi - lo, I, d, K, True, 1e-4, 1e-3, batch_size=B, user_lo=lo,
                        n_slices=n_slices, item_cuts=cuts, store_grad=False, global_user_degree=user_degree)
    del user_degree
    nnz_ui, nnz_iu = len(ui[1]), len(iu[1])
    del ui, iu
    Ug = hi - lo
    # same initialisation as a single-device run of this graph would draw; the item block on every rank
    g = torch.Generator().manual_seed(args.seed)
    bu, bi = (6.0 / (U + d)) ** 0.5, (6.0 / (I + d)) ** 0.5
    for r in range(world):  # the user table is drawn block by block so that no rank holds all of it
        blk = (torch.rand(int(bounds[r + 1] - bounds[r]), d, generator=g) * 2 - 1) * bu
        if r == rank:
            eng.P[:Ug].copy_(blk)
        del blk
    eng.item_rows(eng.P).copy_((torch.rand(I, d, generator=g) * 2 - 1) * bi)
    batches = [eng.make_batch(tri[i * B:(i + 1) * B, 0], tri[i * B:(i + 1) * B, 1], tri[i * B:(i + 1) * B, 2])
               for i in range(n_parity + args.steps + args.warmup + n_timeline)]
    first = n_parity
    last = first + args.warmup + args.steps - 1

    def step(i):
        if i < last:
            eng.prefetch(batches[i + 1])  # index-only work of the next batch, off the critical path
        return eng.train_step(batches[i])

    captured = None
    if n_parity:
        phase("parity_steps")
        captured = parity_capture(eng, batches[:n_parity], tri[:n_parity * B], dist, rank, lo, hi, U, I, seed=args.seed)
    S.ramp_clocks()
    phase("warmup")
    for i in range(first, first + args.warmup):
        step(i)
    dist.barrier()
    torch.cuda.synchronize()
    phase("timed")
    wire0 = dict(comm.wire) if rank_order else None
    t0 = time.perf_counter()
    for i in range(first + args.warmup, first + args.warmup + args.steps):
        step(i)
    t_enqueue = time.perf_counter() - t0  # host time to issue the steps (== wall time when the host is the bottleneck)
    wire1 = dict(comm.wire) if rank_order else None
    eng._wait_item_table()                # (the last step's all-gathers of the updated item rows belong to it)
    torch.cuda.synchronize()
    dist.barrier()
    dt = torch.tensor([time.perf_counter() - t0], dtype=torch.float64,
                      device="cuda" if dist.get_backend() == "nccl" else "cpu")
    dist.all_reduce(dt, op=dist.ReduceOp.MAX)
    dt = float(dt.item())
    phase("after_timed")
    # coherence of the item table (updated by its owners, all-gathered): a checksum must agree on every rank
    chk = eng.item_rows(eng.P).double().sum().reshape(1)
    chk = chk if dist.get_backend() == "nccl" else chk.cpu()
    c_lo, c_hi = chk.clone(), chk.clone()
    dist.all_reduce(c_lo, op=dist.ReduceOp.MIN)
    dist.all_reduce(c_hi, op=dist.ReduceOp.MAX)

    # per-rank roofline of the two products a layer consists of (after the timed region, this rank only)
    def timed(fn, reps=5):
        fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps * 1e-3

    t_ui = timed(lambda: kern.spmm(eng.G_ui, eng._i(eng.P), Y=eng.XU[0]))

    def item_side():
        for gph, r0, r1, r1p in eng.slices:
            kern.spmm(gph, eng._u(eng.P), Y=eng.XI[0][r0:r1])

    t_iu = timed(item_side)
    n_touched = eng.touched_items[1] if eng.touched_items is not None else 0
    # instrumented steps (every rank: they hold collectives): what each collective cost and how long the step's stream
    # waited for it — the diagnosis of a line below the 6x target
    timeline = None
    if n_timeline:
        phase("timeline")
        tl = StepTimeline(torch, world)
        eng._wait_item_table()
        inner, inner_k, eng.comm, eng.timeline = eng.comm, eng.k, TimelineComm(eng.comm, tl), tl
        order = IssueOrder().attach(eng)  # the same steps' launch ORDER, checked against DESIGN.md §7's overlap model
        for i in range(last + 1, last + 1 + n_timeline):
            ev = (tl.event(), tl.event())
            ev[0].record()
            order.begin_step()
            eng.train_step(batches[i])
            ev[1].record()
            tl.steps.append(ev)
        order.end_steps()
        eng._wait_item_table()
        torch.cuda.synchronize()
        eng.comm, eng.k, eng.timeline = inner, inner_k, None
        timeline = tl.summary()
        # every rank checked its own sequence: the line carries rank 0's and the number of ranks that found a violation
        bad = torch.tensor([1.0 if order.violations() else 0.0], device="cuda" if dist.get_backend() == "nccl" else "cpu")
        dist.all_reduce(bad)
        timeline["issue_order"] = dict(order.summary(), ranks_with_violations=int(bad.item()))
        timeline["touched_item_rows_exchanged"] = eng.touched_items[1] if eng.touched_items is not None else 0
        timeline["touched_item_agreement"] = ("device-built id list sized by a host-side bound: no host synchronisation"
                                              if eng.user_degree is not None else "length read back: one host synchronisation")
    rows_form = n_touched > 0
    # panel-sized exchanges per step: forward layers 1..K-2, backward steps 2..K-1 as all-reduces (+ layer K-1 and the
    # first backward step when the touched-item form does not apply), and the last backward step as reduce-scatter +
    # all-gather (the same bytes on the wire as one all-reduce)
    n_allreduce = max(K - 2, 0) + max(K - 2, 0) + (0 if rows_form or K < 2 else 2)
    bytes_ui = 4 * (Ug + 1) + 8 * nnz_ui + 4 * nnz_ui * d + 4 * Ug * d
    bytes_iu = 4 * (I + 1) + 8 * nnz_iu + 4 * nnz_iu * d + 4 * I * d
    # every array of the two products read or written once (the gathered panel once, not once per stored entry)
    bytes_min = 4 * (Ug + I + 2) + 8 * (nnz_ui + nnz_iu) + 2 * 4 * (Ug + I) * d
    out = None
    if rank == 0:
        out = {
            "metric": "BPR triples/sec, LightGCN-%d dim=%d" % (K, d),
            "value": B * args.steps / dt, "unit": "triples/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "strong",
            "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": "%s graph cut across %d ranks by nnz-balanced user-row blocks: %d users x %d items, %d train "
                                   "edges, nnz(A)=%d; LightGCN K=%d d=%d, ONE global batch of B=%d triples per Adam step (as "
                                   "the reference, trainer.py:36); item table replicated, its Adam state and update owned 1/%d "
                                   "per rank; per step %d all-reduces of the [%d,%d] fp32 item panel in %d slices + 1 "
                                   "reduce-scatter and 1 all-gather of it (the last backward product: owners finish the "
                                   "gradient, apply Adam and send the updated rows round under the next step's first "
                                   "product) + 2 of [%d,%d] (the batch's user rows) + 1 of [<=%d,%d] (the last forward "
                                   "layer's item rows)%s over %s"
                                   % (args.workload, world, U, I, n_edges, nnz_global, K, d, B, world, n_allreduce, I, d,
                                      len(eng.slices), B, d, 2 * B, d,
                                      (" + the %d item rows the batch's users touch, for forward layer K-1 and the first "
                                       "backward product (an [%d] flag vector to agree on them, then those rows)"
                                       % (n_touched, I)) * rows_form,
                                      "RCCL" if dist.get_backend() == "nccl" else dist.get_backend() + " (rehearsal, host-staged)"),
                       "batch": B, "dim": d, "layers": K, "parallelism": "user-row shard x%d" % world,
                       "comm": comm_name, "item_panel_slices": len(eng.slices)},
            "loss_last": [float(x) for x in eng.loss.cpu()],
            "host_issue_ms_per_step": t_enqueue / args.steps * 1e3,
            "item_table_coherent": bool(c_lo.item() == c_hi.item()),
            "timeline": timeline,
            # per-step work every rank carries whatever N is (what caps the speed-up before any communication): O(I + B d)
            "replicated_bytes_per_step_per_rank": eng.replicated_bytes_per_step(),
            "roofline": {
                "bound": "hbm", "kernel": "spmm_tile_kernel<%d,...> on rank 0's two blocks: R_g (users x items) and R_g^T "
                                          "(items x users, %d row slices)" % (min(d // 4, 64), len(eng.slices)),
                "achieved": (bytes_ui + bytes_iu) / (t_ui + t_iu) / 1e9, "peak": 8000.0, "unit": "GB/s",
                "frac": (bytes_ui + bytes_iu) / (t_ui + t_iu) / 1e9 / 8000.0, "traffic": None,
                "us_user_side": t_ui * 1e6, "us_item_side": t_iu * 1e6, "bytes_gather_user_side": bytes_ui,
                "bytes_gather_item_side": bytes_iu, "bytes_min": bytes_min,
                "frac_bytes_min": bytes_min / (t_ui + t_iu) / 1e9 / 8000.0, "rank0_users": Ug, "rank0_nnz": nnz_ui,
                "cache_resident": bool(4 * max(I, Ug) * d < (256 << 20)),
                # bytes a rank sends (= receives) per step: an all-reduce or a reduce-scatter + all-gather pair moves
                # 2 (N-1)/N of the buffer per rank
                "exchange_bytes_per_step_per_rank": int(2 * (world - 1) / world *
                                                        ((n_allreduce + 1) * 4 * I * d + 3 * 4 * B * d
                                                         + (2 * 4 * n_touched * d + 4 * I) * rows_form)),
                "exchange_rows": {"touched_items": n_touched, "items": I},
            },
        }
        # bytes one rank puts on the wire per step (SURVEY.md 8e / DESIGN.md 7: what the 1 -> 8 speed-up hangs on)
        fp32_wire = out["roofline"]["exchange_bytes_per_step_per_rank"]
        out["panel_exchange"] = {"bits": panel_bits, "bytes_on_the_wire_per_step_per_rank": fp32_wire,
                                 "reduction_order": "RCCL's (ring / tree by its own choice)"}
        if rank_order:
            sent = (wire1["packed_bytes_sent"] - wire0["packed_bytes_sent"]) / args.steps
            repl = (wire1["fp32_bytes_it_replaces"] - wire0["fp32_bytes_it_replaces"]) / args.steps
            out["panel_exchange"].update(
                bytes_on_the_wire_per_step_per_rank=int(fp32_wire - repl + sent), packed_bytes_per_step_per_rank=int(sent),
                fp32_bytes_they_replace=int(repl), ratio=(sent / repl) if repl else None,
                exchanges_per_step=(wire1["exchanges"] - wire0["exchanges"]) / args.steps,
                reduction_order="rank order (%s: q0 + q1 + ... one fp32 add per rank and element): bit-reproducible run to run"
                                % ("idg_reduce24_f32" if panel_bits == 24 else "idg_reduce_blocks_f32"),
                order_violations=comm.order_violations(),
                what=("the [I, d] all-reduces, the last backward product's reduce-scatter, the all-gather of the updated item rows "
                      "and the touched-item row sets travel as 24-bit values (2^-16 relative), 3 bytes per value; the batch's guest "
                      "rows and other small collectives stay fp32") if panel_bits == 24 else
                     ("the [I, d] all-reduces, the last backward product's reduce-scatter and the touched-item row sets as an explicit "
                      "exchange of fp32 blocks (all-to-all, this library's rank-ordered sum, all-gather): RCCL's bytes, a fixed order"))
    kern.close()
    if rank_order:
        comm.release_buffers()
    del eng, batches, kern
    torch.cuda.empty_cache()
    phase("single_gpu_reference")
    if single_gpu_reference is not None:
        # the SAME workload unsharded on ONE GPU, measured in this run (rank 0; the other ranks wait at the barrier)
        ref = None
        if rank == 0:
            try:
                ref = single_gpu_reference(args, edges, captured)
            except Exception as exc:  # noqa: BLE001 - the headline stands without it; the line says why it is missing
                ref = {"error": "%s: %s" % (type(exc).__name__, str(exc)[:200])}
            out["single_gpu_reference"] = ref
            if n_parity:
                # correctness of the N-rank run, in the line itself: ok = False makes bench.py leave with a non-zero status
                out["parity_vs_1gpu"] = ref.pop("parity_vs_1gpu", None) or {
                    "ok": None, "error": "the single-GPU reference did not run: " + str(ref.get("error", "no result"))}
            if ref.get("ms_per_step"):
                out["speedup_vs_1gpu"] = ref["ms_per_step"] / out["ms_per_step"]
                if world >= 8 and out["speedup_vs_1gpu"] < 6.0:
                    out["north_star_6x"] = ("NOT met: %.2fx at %d GPUs with exact fp32 panels — three [I, d] exchanges per step "
                                            "(%.1f GB sent per rank) against %.0f ms of products per rank"
                                            % (out["speedup_vs_1gpu"], world,
                                               out["roofline"]["exchange_bytes_per_step_per_rank"] / 1e9,
                                               ref["ms_per_step"] / world))
        dist.barrier()
    return out
