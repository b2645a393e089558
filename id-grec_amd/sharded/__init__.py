"""The user-row-sharded LightGCN training step across the GPUs of one node, as a package.

    partition.py    the nnz partitioner and the shard extraction (numpy only)
    step.py         GlobalBatch, ShardedEngine: the algorithm (its statement is that module's docstring)
    instruments.py  StepTimeline / TimelineComm (per-collective timing) and IssueOrder / OrderComm / OrderKernels (the host
                    issue order as a checked property): wrappers around a comm and a kernels object
    kernels.py      HipKernels: `kernels` bound to libidgrec.so
    comm.py         TorchComm, NativeComm (RCCL), make_comm (the choice between them), NoComm (world size 1)
    packed.py       Packed24Comm / RankOrderComm: the panel exchanges as an explicit, rank-ordered exchange (opt-in)
    driver.py       `bench.py --gpus N`: run_sharded_bench with parity_capture / parity_compare

Only driver.py imports its siblings.  The others meet through the two objects handed to ShardedEngine (and to
Packed24Comm), so the world_size-2 gloo tests in tests/ drive the layer loop on CPU with a checker-backed stub that honours
the same bitmaps (and poisons every row a restricted product does not produce), while the product binds it to the HIP
kernels (`HipKernels`) and RCCL (`NativeComm` / `TorchComm`).  Importing this package loads none of torch, native, ops or
synth: those are imported inside the functions that need them.

`comm` — collectives over the ranks; buffers are fp32 arrays of whatever `kernels` allocates; every *_async returns a
handle (or None) for wait():
    all_reduce_async(t, average=False)   t <- the sum over ranks (the mean only if asked AND comm.averages)
    all_gather_async(out, t)             out (world blocks, rank-major) <- every rank's t; t may be this rank's block of out
    reduce_scatter_async(t)              t = world equal blocks; this rank's block <- the sum over ranks of it, in place
    all_to_all_async(recv, send)         block p of send goes to rank p, block p of recv comes from rank p (Packed24Comm's
                                         inner comm only; the step itself never calls it)
    wait(handle)                         the current stream (or the host) goes on once the collective is done
    world, rank                          ints
    averages                             whether average=True is honoured inside the collective
    tag, slice                           set by ShardedEngine before every collective: what it is ("F1.panel", "guest_rows",
                                         "item_table.all_gather", ...) and which item slice; the instruments read them
  optional (read through getattr):
    packed                               True: the replicated item table holds 24-bit values, the owner keeps an fp32 master
    by_blocks                            True: sliced all-reduces get the padded slice (one equal block per rank)
    packed_target(t, n_valid)            the send buffer of the next exchange of t for a product that writes it packed, or None
    timed_stream(nbytes)                 the torch stream a collective of that size runs on if not the current one (TimelineComm)
    wire_bytes(numel)                    bytes on the wire for that many values (TimelineComm's bus rate)
    order_violations()                   a compound exchange's own order check, as strings (IssueOrder adds them to its own)

`kernels` — allocation, the products and the row kernels; called by ShardedEngine:
    zeros(shape), fill(a, v), to_device(numpy array), make_graph(indptr, indices, values, n_rows, n_cols)
    spmm(graph, X, Y=, addend=, sums=, sum_out=, div=, accumulate=, mask=, adam=, out_rows=, x_rows=, discard_grad=, Y24=)
                                         the product with its fused epilogue, restricted by row / input bitmaps
    bits_from(bits, row0), ones_bits(n)  a bitmap from row row0 on (a multiple of 32); an all-ones bitmap
    prepare(eng, gb) -> prep, wait_rows(prep), release(prep)
                                         the batch's index-only work (bitmaps own_users / items, scatter plan), maybe ahead
    touched_local(eng, prep, gb), flag_touched_items(eng, prep, gb, flags), compact_ids(flags, n), nonzero_ids(flags),
    touched_from_ids(eng, prep, ids, n)  the touched-item agreement: set prep.touched and prep.near
    gather_rows(dst, src, idx), gather_rows2(dst0, src0, dst1, src1, idx), scatter_rows(dst, idx, src),
    chain_rows2(dst0, src0, dst1, src1, idx, nxt, store)
                                         row movers (guest rows, compact row sets, gradients going home in batch order)
    layer_mean(out, ids, terms, last, div), bpr(fin, ego, n_users, users, pos, neg, reg_lambda, g_final, g_ego, loss, prep)
    item_tail(t, g, G, live_bits, row0, c0, cnt, store_grad, p, m, v, lr, step), adam(p, g, m, v, lr, step)
    topk(user_panel, item_panel, users, k, excl_indptr, excl_items)          evaluation
  called by Packed24Comm:
    zeros, pack24(src, dst, n), unpack24(src, dst, n), reduce24(blocks, n_blocks, n, out_packed=, out_f32=),
    reduce_blocks(blocks, n_blocks, n, out), exchange_stream() (context manager), record_event(), wait_event(ev)
"""
from .comm import NativeComm, NoComm, TorchComm, make_comm
from .driver import PARITY_TOL, parity_capture, parity_compare, run_sharded_bench
from .instruments import XGMI_PEAK_GBS, IssueOrder, OrderComm, OrderKernels, StepTimeline, TimelineComm
from .kernels import HipKernels
from .packed import Packed24Comm, RankOrderComm
from .partition import partition_users_by_nnz, shard_adjacency, shard_adjacency_from_edges
from .step import GlobalBatch, ShardedEngine

__all__ = [
    "GlobalBatch", "HipKernels", "IssueOrder", "NativeComm", "NoComm", "OrderComm", "OrderKernels", "PARITY_TOL",
    "Packed24Comm", "RankOrderComm", "ShardedEngine", "StepTimeline", "TimelineComm", "TorchComm", "XGMI_PEAK_GBS",
    "make_comm", "parity_capture", "parity_compare", "partition_users_by_nnz", "run_sharded_bench", "shard_adjacency",
    "shard_adjacency_from_edges",
]
