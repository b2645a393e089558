"""PropagationEngine's training step in every form of loss_and_grad on a fixed small graph (1000 users x 640 items, ~30000
edges from synth; d = 64, two seeds): four train_steps over batches of 256, 256, 256 and 100 triples (duplicate ids; the
short last batch re-allocates the slot's workspaces), each form with and without prefetch and with fuse_adam on and off.
Forms: plain (IDG_STEP_PLAN=0 is set here: the call-by-call chain), ssl, xssl with K = 2 without layer 0 (the Horner
branch) and with it (the fallback), sgl on two edge-dropped copies of the graph, au, sccf, na with and without BPR; and
with graph=None: plain, au, sccf, both na forms.
Prints, per deterministic run, a checksum of the raw bits of params, grad, the four loss vectors and the touched bitmap;
per float-atomic run (deterministic=False) the losses to four significant digits.  Under IDG_PACE=0 — the waits then do
not depend on timing — also a checksum of the run's call trace: every ops.*_raw function, every Graph method and
LocalEvent.record / wait / synchronize / query, each with the stream it names (main or side); two steps of NGCF and of
BIGCF (BatchPrep engines) are traced the same way.  An argument names a file that receives the traces in full.
Imports the tree it lies in: copy it into another revision's tree, run both with the same library (IDG_LIB_PATH); equal
lines = the two trees launch and compute the same."""
import hashlib
import os
import sys
import tempfile
import types

os.environ["IDG_STEP_PLAN"] = "0"
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import idgrec_amd.host as H  # noqa: E402
import idgrec_amd.synth as S  # noqa: E402
from idgrec_amd import ops  # noqa: E402
from idgrec_amd.engine import PropagationEngine  # noqa: E402

U, I, E, d = 1000, 640, 30000, 64
SIZES = (256, 256, 256, 100)
TRACING = os.environ.get("IDG_PACE", "1") == "0"
trace, side_streams = [], set()
dump = open(sys.argv[1], "w") if len(sys.argv) > 1 else None


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(b"none" if t is None else t.detach().cpu().numpy().tobytes())
    return h.hexdigest()[:12]


def traced(name, fn, stream_arg=None):
    """fn, logging `name` and the stream the call names: its `stream` keyword, or positional argument stream_arg."""
    def call(*a, **kw):
        s = kw.get("stream") if stream_arg is None else a[stream_arg]
        trace.append("%s %s" % (name, "side" if s in side_streams else "main"))
        return fn(*a, **kw)
    return call


def install_trace():
    # a *_raw function is patched wherever its object is bound: idgrec_amd.ops and, where ops is a package, its submodules
    # (the module that defines it and those that import it), so a call one wrapper makes to another is traced in both trees
    homes = [m for key, m in sorted(sys.modules.items())
             if m is not None and (key == ops.__name__ or key.startswith(ops.__name__ + "."))]
    for name, fn in list(vars(ops).items()):
        if name.endswith("_raw") and isinstance(fn, types.FunctionType):
            call = traced(name, fn)
            for m in homes:
                if vars(m).get(name) is fn:
                    setattr(m, name, call)
    for name, fn in list(vars(ops.Graph).items()):
        if isinstance(fn, types.FunctionType) and not name.startswith("_"):
            setattr(ops.Graph, name, traced("Graph." + name, fn))
    for name in ("record", "wait"):
        setattr(ops.LocalEvent, name, traced("LocalEvent." + name, getattr(ops.LocalEvent, name), stream_arg=1))
    for name in ("synchronize", "query"):
        setattr(ops.LocalEvent, name, traced("LocalEvent." + name, getattr(ops.LocalEvent, name)))
    make = ops.side_stream

    def side_stream(device):
        s = make(device)
        side_streams.add(s.cuda_stream)
        return s
    ops.side_stream = side_stream


def end_trace(label):
    if TRACING:
        print("%s trace %d calls %s" % (label, len(trace), hashlib.sha256("\n".join(trace).encode()).hexdigest()[:12]), flush=True)
        if dump is not None:
            dump.write("== %s\n%s\n" % (label, "\n".join(trace)))
    del trace[:]


if TRACING:
    install_trace()
users, items = S.generate(U, I, E, seed=0)
ip, ix, dv = H.build_norm_adj(U, I, users, items)
n = U + I
G = ops.Graph(ip, ix, dv, n, n)
# two edge-dropped views on the graph's own schedule: the (row, col) and (col, row) entries of an edge fall together
row = np.repeat(np.arange(n, dtype=np.int64), np.diff(ip))
edge = np.minimum(row, ix) * n + np.maximum(row, ix)
d_ip, d_ix = torch.from_numpy(ip.astype(np.int64)).cuda(), torch.from_numpy(ix.astype(np.int32)).cuda()
subs = [G.revalued_copy(d_ip, d_ix, torch.from_numpy((dv * ((edge * 2654435761 + salt) % 10 != 0)).astype(np.float32)).cuda())
        for salt in (1, 2)]

SSL = (0.1, 0.2, 0.1)
NA_BPR, NA_ALONE = (0.2, 0.1, None, True), (0.2, 0.1, 0.5, False)
FORMS = [  # (name, graph, K, include_layer0, mode attributes, also with float atomics)
    ("plain", G, 3, True, {}, True),
    ("ssl", G, 3, False, {"ssl": SSL}, False),
    ("xssl horner", G, 2, False, {"xssl": SSL}, False),
    ("xssl fallback", G, 2, True, {"xssl": SSL}, False),
    ("sgl", G, 3, True, {"sgl": (0.2, 0.1, subs[0], subs[1])}, False),
    ("au", G, 3, True, {"au": (2.0,)}, True),
    ("sccf", G, 3, True, {"sccf": (0.2,)}, True),
    ("na+bpr", G, 3, True, {"na": NA_BPR}, True),
    ("na alone", G, 3, True, {"na": NA_ALONE}, True),
    ("mf plain", None, 0, True, {}, True),
    ("mf au", None, 0, True, {"au": (2.0,)}, True),
    ("mf sccf", None, 0, True, {"sccf": (0.2,)}, True),
    ("mf na+bpr", None, 0, True, {"na": NA_BPR}, True),
    ("mf na alone", None, 0, True, {"na": NA_ALONE}, True),
]


def run(form, W, batches, deterministic, prefetch, fuse_adam):
    _, graph, K, inc, modes, _ = form
    torch.manual_seed(2024)
    ops.reset_noise_stream()
    eng = PropagationEngine(graph, U, I, d, K, include_layer0=inc, reg_lambda=1e-4, lr=1e-3, deterministic=deterministic,
                            params=W.clone())
    eng.fuse_adam = fuse_adam
    for k, v in modes.items():
        setattr(eng, k, v)
    losses = []
    if prefetch:
        eng.prefetch(*batches[0])
    for s, b in enumerate(batches):
        if prefetch and s + 1 < len(batches):
            eng.prefetch(*batches[s + 1])
        losses.append(eng.train_step(*b).clone())
    torch.cuda.synchronize()
    return eng, losses


for seed in (0, 1):
    tri = torch.from_numpy(S.draw_triples(seed, users, items, U, I, sum(SIZES))[0][:sum(SIZES)].copy())
    tri[1::7] = tri[0::7][: len(tri[1::7])]  # duplicate triples next to the duplicate ids a batch of 256 has anyway
    tri = tri.cuda()
    cuts = np.concatenate([[0], np.cumsum(SIZES)])
    batches = [tuple(tri[a:b, c].contiguous() for c in range(3)) for a, b in zip(cuts[:-1], cuts[1:])]
    g = torch.Generator().manual_seed(seed)
    W = torch.cat([(torch.rand(U, d, generator=g) * 2 - 1) * (6.0 / (U + d)) ** 0.5,
                   (torch.rand(I, d, generator=g) * 2 - 1) * (6.0 / (I + d)) ** 0.5]).cuda()
    for form in FORMS:
        for prefetch in (False, True):
            for fuse_adam in (True, False):
                label = "seed %d  %-13s prefetch %d fuse_adam %d " % (seed, form[0], prefetch, fuse_adam)
                eng, losses = run(form, W, batches, True, prefetch, fuse_adam)
                print("%s params %s  grad %s  loss %s  touched %s" % (label, digest(eng.params), digest(eng.grad),
                                                                       digest(*losses), digest(eng.touched)), flush=True)
                del eng
                end_trace(label)
        if form[5]:
            eng, losses = run(form, W, batches, False, False, True)
            print("seed %d  %-13s atomics  losses %s" % (seed, form[0], "  ".join(
                "[" + " ".join("%.4g" % v for v in l.tolist()) + "]" for l in losses)), flush=True)
            del eng
            end_trace("seed %d  %-13s atomics" % (seed, form[0]))

if TRACING:  # two steps (the second prepared ahead) of two engines that hold a BatchPrep
    import importlib

    import utility.utility_data.data_loader as data_loader
    import utility.utility_function.tools as tools

    root = tempfile.mkdtemp(prefix="idg_engine_ab_")
    S.make_dataset(root, "small", shape=(U, I, E), n_test=1)
    for name in ("NGCF", "BIGCF"):
        cfg = tools.read_configuration(os.path.join(ROOT, "configure", name + ".txt"), name)
        cfg.update(dataset="small", dataset_path=root + "/", sparsity_test="0")
        data = data_loader.Data(os.path.join(root, "small"), cfg)
        tools.set_seed(2024)
        ops.reset_noise_stream()
        m = getattr(importlib.import_module("models." + name), name)(cfg, data, torch.device("cuda")).to("cuda")
        assert m.fused_step_available()
        opt = ops.Adam(list(m.parameters()), lr=float(cfg["learn_rate"]))
        out = torch.zeros(2, m.n_fused_losses, device="cuda")
        del trace[:]
        for s in range(2):
            if s == 0:
                m.prefetch_batch(*batches[1])
            assert m.fused_train_step(*batches[s], out[s], opt)
        torch.cuda.synchronize()
        print("%-5s loss %s" % (name, digest(out)), flush=True)
        end_trace(name)
