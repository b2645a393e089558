"""IMP-GCN on the device: the two kernels of idgrec_amd/csrc/idg_group.hip, ops.grouped_propagate, the fused chain of
idgrec_amd/impgcn.py and the plugin, against tests/impgcn_ref64.py in float64.  Every float comparison is the rule of
egcf_ref64.band(): the kernel may sit up to four times as far from float64 as the SAME expressions in float32 torch do
(floored at 8 * 2^-24), both distances printed.  Memberships are compared exactly, except on rows that assign64 flags as
near-tied (a correct float32 evaluation may choose differently there); those rows are counted and bounded.

  (a) idg_group_assign_f32: n in {1, 63, 64, 65, 130, 32 833} x G in {1, 2, 3, 8} x p in {0, 0.4} x num_users in {0, n / 2, n};
      constructed ties; guards around both outputs
  (b) idg_grouped_spmm_f32 on graph_tiny, graph_small and a constructed bipartite graph (one item row of 1 500 entries — three
      chunks, the long-row kernels — one empty user row, one empty item row): shared / grouped X, with / without V, Y / S /
      both, S_in; five kinds of membership; NaN in every row that must not be read, NaN where nothing may be written
  (c) equal bits run to run, and with / without the long-row schedule
  (d) ops.grouped_propagate under autograd at d = 64 (the raw calls' bits) and d = 128 (the composition)
  (e) ImpgcnEngine: two consecutive steps with different batches, (G, L) in {(3, 6), (2, 3), (3, 1)} x p in {0, 0.4}
  (f) models.IMPGCN against the reference's goldens (tolerances of test_gpu_gccf.py::test_model_matches_reference_goldens)
  (g) the optimizer hand-off, as tests/test_gpu_engine_handoff.py asks of the other engines

Measured on one MI355X (e_kernel / e_f32 as fractions of the tensor's largest entry; in brackets the worst share of the band):
  (a) scores: e_kernel at most 4.0e-7 next to e_f32 = 2.4e-7 (0.41: n = 1, G = 2, p = 0); near-tied rows 0 or 1 of 32 833, none below;
      multi-group users at p = 0.4, G = 3: 0.223 of 32 833 (0.154 .. 0.238 at n = 63 .. 130; not asserted there)
  (b) Y and S at most 0.24 of the band; next to ops.spmm with every group for everyone: inside the band both ways
  (e) losses, final, GRAD at most 0.33 of the band (G = 2, L = 3, p = 0.4, step 1, the BPR loss); Adam moments at most
      2.22 * 2^-24 of their largest entry
  (f) trajectory: no element outside rtol 1e-4 / atol 1e-6, at most 4.4e-7 from the reference's tables
Value-only breaks of a scratch copy of the library (valid memory, ordinary failures), one run of this file each, tests failing:
  the column mask is ignored (every entry counts as shared)       18  ((b) but `one` and `all`, where the column mask is
      no restriction; the bitmaps; (d) at d = 64; (e) but L = 1, which has no product; both of (f))
  ties are resolved to the first maximum only                      11  ((a) at n >= 63 — the one row of n = 1 has no tie —
      and the constructed ties; (e) at p = 0.4; both of (f))
  both dropouts use one stream                                     13  (all of (a), the constructed ties and the mask test;
      (e) at p = 0.4; both of (f))
"""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import impgcn_ref64 as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = torch.float32, torch.float64
NAN = float("nan")
D = 64
SEED = 0x1234567890ABCDEF  # (does not fit 32 bits)
REG, LR = 1e-4, 1e-3


@pytest.fixture(scope="module")
def ops():
    import idgrec_amd.ops as ops_

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return ops_


@pytest.fixture(scope="module")
def golden_impgcn():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "impgcn_small.npz"), allow_pickle=False))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rng(*key):
    import zlib

    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _randn(rng, shape, scale=1.0):
    return dev((rng.standard_normal(shape) * scale).astype(np.float32))


def _check(what, got, ref64, f32, quiet=False):
    e_k, e_f = ref.errors(got, ref64, f32)
    if not quiet:
        print("  %-78s e_kernel %.2e  e_f32 %.2e  (%.2f of the band)" % (what, e_k, e_f, e_k / ref.band(e_f)))
    assert e_k <= ref.band(e_f), "%s: e_kernel %.3e above max(4 e_f32 = %.3e, %.3e)" % (what, e_k, 4 * e_f, ref.FLOOR)
    return e_k, e_f


def _bitmap(n, rows):
    rows = np.asarray(rows, dtype=np.int64)
    words = np.zeros((n + 31) // 32, dtype=np.uint32)
    np.bitwise_or.at(words, rows >> 5, np.uint32(1) << (rows & 31).astype(np.uint32))
    return dev(words.view(np.int32))


def _linear(rng, out, inp):
    """nn.Linear's default init: weight and bias uniform in +- 1 / sqrt(in)."""
    k = 1.0 / np.sqrt(inp)
    return dev(rng.uniform(-k, k, (out, inp)).astype(np.float32)), dev(rng.uniform(-k, k, out).astype(np.float32))


# ===================================================================================================== (a) the assignment
ASSIGN_N = [1, 63, 64, 65, 130, 32833]
GUARD = 64


def _guarded(n_elems, dtype, pattern):
    """A buffer with GUARD elements of `pattern` on both sides of the n_elems the kernel may write (pre-filled too)."""
    buf = torch.full((n_elems + 2 * GUARD,), pattern, dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + n_elems]


@pytest.mark.parametrize("n", ASSIGN_N)
def test_assignment_vs_float64(ops, n):
    rng = _rng("assign", n)
    ego, side = _randn(rng, (n, D), 0.1), _randn(rng, (n, D), 0.1)
    Wfc, bfc = _linear(rng, D, D)
    mask1 = {0.0: None, 0.4: ref.keep_mask(0.4, SEED, 5, n, D).cuda()}
    for G in (1, 2, 3, 8):
        Wgrp, bgrp = _linear(rng, G, D)
        for p in (0.0, 0.4):
            m2 = None if p == 0 else ref.keep_mask(p, SEED, 9, n, G).cuda()
            want = {}
            for name, dtype in (("64", F64), ("32", F32)):
                cast = lambda t: None if t is None else t.to(dtype)  # noqa: E731
                want[name] = ref.assign64(ego, side, Wfc, bfc, Wgrp, bgrp, n, cast(mask1[p]), cast(m2), dtype=dtype)
            scores64, member64, near = want["64"]
            for nu in sorted({0, n // 2, n}):
                tag = "assign n=%d G=%d p=%g num_users=%d" % (n, G, p, nu)
                mbuf, member = _guarded(n, torch.uint8, 0xA5)
                sbuf, scores = _guarded(n * G, F32, NAN)
                scores = scores.view(n, G)
                got = ops.group_assign_raw(ego, side, Wfc, bfc, Wgrp, bgrp, nu, p, SEED, 5, 9, member=member, scores_out=scores)
                assert got.data_ptr() == member.data_ptr()
                assert (mbuf[:GUARD] == 0xA5).all() and (mbuf[GUARD + n:] == 0xA5).all(), tag + ": bytes around member"
                assert torch.isnan(sbuf[:GUARD]).all() and torch.isnan(sbuf[GUARD + n * G:]).all(), tag + ": floats around scores_out"
                assert torch.isfinite(scores).all()
                _check(tag + " scores", scores, scores64, want["32"][0], quiet=nu != n)
                # exact, ties included: the membership IS the arg-max set of the scores the kernel compared
                assert torch.equal(member, ref.argmax_set(scores, nu)), tag + ": member is not the arg-max set of scores_out"
                assert (member[nu:] == (1 << G) - 1).all(), tag + ": item rows"
                users_near = int(near[:nu].sum())
                assert users_near <= 0.005 * n, "%s: %d near-tied rows" % (tag, users_near)
                same = (member[:nu] == member64[:nu]) | near[:nu]
                assert bool(same.all()), "%s: %d rows differ from float64's membership" % (tag, int((~same).sum()))
                if nu and G > 1:
                    multi = float(((member[:nu] & (member[:nu] - 1)) != 0).float().mean())
                    if nu == n:
                        print("  %-78s multi-group users %.3f, near-tied rows %d" % (tag, multi, users_near))
                    if p == 0:
                        assert multi == 0.0  # no dropout, no exact tie among random scores
                    elif G == 3 and nu >= 1000:
                        # the issue's band for Dropout(0.4) on three scores.  A smaller sample is not held to it: 65 users
                        # put one standard deviation of a share of 0.2 at 0.05
                        assert 0.1 < multi < 0.3, tag


def test_assignment_constructed_ties(ops):
    """W_fc = I, b_fc = 0, side = 0 and positive rows make temp = ego; W_grp's rows then pick the scores by hand."""
    n, G = 6, 3
    ego = torch.zeros(n, D, device="cuda")
    eye, zero = torch.eye(D, device="cuda"), torch.zeros(D, device="cuda")
    Wgrp = torch.zeros(G, D, device="cuda")
    Wgrp[0, 0], Wgrp[1, 1], Wgrp[2, 2] = 1.0, 1.0, 1.0
    bgrp = torch.zeros(G, device="cuda")
    ego[0, :3] = torch.tensor([2.5, 1.0, 2.5])   # two equal positive scores
    ego[1, :3] = torch.tensor([0.0, 0.0, 0.0])   # all zero
    ego[2, :3] = torch.tensor([1.0, 3.0, 2.0])   # a single maximum
    ego[3, :3] = torch.tensor([4.0, 4.0, 4.0])
    ego[5, :3] = torch.tensor([1.0, 3.0, 2.0])   # an item row
    scores = torch.empty(n, G, device="cuda")
    member = ops.group_assign_raw(ego, torch.zeros_like(ego), eye, zero, Wgrp, bgrp, 5, 0.0, 1, 2, 3, scores_out=scores)
    assert member.tolist() == [0b101, 0b111, 0b010, 0b111, 0b111, 0b111]
    # -0.0 against +0.0: group 0's weights and bias are all -0.0 — products of -0.0 with temp >= 0 and their sums stay -0.0 —
    # group 1's +0.0, group 2's score is -1
    wz = torch.zeros(G, D, device="cuda")
    wz[0] = -0.0
    bz = torch.tensor([-0.0, 0.0, -1.0], device="cuda")
    member = ops.group_assign_raw(ego, torch.zeros_like(ego), eye, zero, wz, bz, 5, 0.0, 1, 2, 3, scores_out=scores)
    assert torch.signbit(scores[0, 0]) and not torch.signbit(scores[0, 1]) and float(scores[0, 0]) == 0.0
    assert member.tolist() == [0b011] * 5 + [0b111]
    # all scores dropped -> all groups: negative biases, p = 0.4; the rows whose three keep values are all 0 are full, and a
    # row with one survivor (negative) and two dropped scores ties on the two zeros
    n = 4096
    ego = torch.zeros(n, D, device="cuda")
    bneg = torch.tensor([-1.0, -2.0, -3.0], device="cuda")
    scores = torch.empty(n, G, device="cuda")
    member = ops.group_assign_raw(ego, ego.clone(), eye, zero, torch.zeros(G, D, device="cuda"), bneg, n, 0.4, SEED, 5, 9, scores_out=scores)
    keep = ref.keep_mask(0.4, SEED, 9, n, G).cuda() != 0
    want = torch.where(keep.all(dim=1), torch.tensor(1, device="cuda"), ref.bits_of(~keep).long()).to(torch.uint8)
    assert torch.equal(member, want)
    assert int((member == 0b111).sum()) == int((~keep).all(dim=1).sum()) > 100
    assert torch.equal(scores, (bneg.double()[None, :] * ref.keep_mask(0.4, SEED, 9, n, G).cuda()).float())


def test_the_two_masks_are_the_published_ones_of_their_own_streams(ops):
    """W_fc = I, b_fc = 0, side = 0, ego = 1: temp = keep1.  W_grp = rows of ones, b_grp = 0, p for the second mask the same:
    scores[r, g] = keep2[r, g] * sum_f keep1[r, f] — exact in float32 (sums of at most 64 equal numbers 1 / 0.6)."""
    n, G, p = 257, 3, 0.4
    one = torch.ones(n, D, device="cuda")
    scores = torch.empty(n, G, device="cuda")
    ops.group_assign_raw(one, torch.zeros_like(one), torch.eye(D, device="cuda"), torch.zeros(D, device="cuda"),
                         torch.ones(G, D, device="cuda"), torch.zeros(G, device="cuda"), n, p, SEED, 5, 9, scores_out=scores)
    k1, k2 = ref.keep_mask(p, SEED, 5, n, D).cuda(), ref.keep_mask(p, SEED, 9, n, G).cuda()
    want = k2 * k1.sum(dim=1, keepdim=True)
    assert float((scores.double() - want).abs().max()) <= 64 * 2.0 ** -22 * float(want.max())
    assert torch.equal(scores == 0, want == 0)
    # one stream for both masks would give keep2[r, g] = keep1[r, g]
    other = ref.keep_mask(p, SEED, 5, n, G).cuda() * k1.sum(dim=1, keepdim=True)
    assert not torch.equal(scores == 0, other == 0)


# ================================================================================================= (b) the grouped product
def _constructed():
    """2 000 nodes, bipartite and symmetric: 1 600 users, 400 items.  Item 0 has 1 500 entries (three chunks of 512: the
    long-row kernels); the last user and the last item have none; every other user has 1 .. 8 further items."""
    rng = _rng("constructed graph")
    U, I = 1600, 400
    pairs = {(u, 0) for u in range(1500)}          # item 0: 1 500 users — three chunks of 512
    for u in range(U - 1):                          # (user U - 1 stays empty)
        for i in rng.choice(np.arange(1, I - 1), size=int(rng.integers(1, 9)), replace=False):  # (item I - 1 stays empty)
            pairs.add((u, int(i)))
    import scipy.sparse as sp

    uu, ii = np.array(sorted(pairs)).T
    R = sp.csr_matrix((np.ones(len(uu), dtype=np.float64), (uu, ii)), shape=(U, I))
    A = sp.bmat([[None, R], [R.T, None]]).tocsr()
    deg = np.asarray(A.sum(axis=1)).reshape(-1)
    dinv = np.where(deg > 0, 1.0 / np.sqrt(np.maximum(deg, 1)), 0.0)
    A = (sp.diags(dinv) @ A @ sp.diags(dinv)).tocsr().astype(np.float32)
    A.sort_indices()
    lens = np.diff(A.indptr)
    assert lens[U] == 1500 and lens[U - 1] == 0 and lens[U + I - 1] == 0 and (lens[:U - 1] > 0).all()
    return dict(adj_indptr=A.indptr.astype(np.int64), adj_indices=A.indices.astype(np.int32), adj_data=A.data, num_users=U, num_items=I)


_cases = {}


def _graph_case(ops, name, golden_tiny, golden_small):
    if name not in _cases:
        g = {"tiny": golden_tiny, "small": golden_small}.get(name) or _constructed()
        U, I = int(g["num_users"]), int(g["num_items"])
        n = U + I
        graph = ops.Graph(g["adj_indptr"], g["adj_indices"], g["adj_data"], n, n)
        csr = ops.GroupCsr(g["adj_indptr"], g["adj_indices"], g["adj_data"], n, "cuda", graph=graph)
        plain = ops.GroupCsr(g["adj_indptr"], g["adj_indices"], g["adj_data"], n, "cuda", schedule=False)
        A64 = ref.dense_operator(g["adj_indptr"], g["adj_indices"], g["adj_data"], (n, n), device="cuda")
        _cases[name] = (U, n, graph, csr, plain, A64)
    return _cases[name]


MEMBERSHIPS = ("one", "all", "single", "multi", "zero")


def _membership(kind, U, n, G, rng):
    m = np.full(n, (1 << G) - 1, dtype=np.uint8)
    if kind == "one":      # one group for everyone (items too: D_g is the identity for g = 1, zero for the others)
        m[:] = 0b010 if G > 1 else 1
    elif kind == "single":
        m[:U] = 1 << rng.integers(0, G, U)
    elif kind in ("multi", "zero"):
        m[:U] = 1 << rng.integers(0, G, U)
        extra = rng.random(U) < 0.2
        m[:U] = np.where(extra, m[:U] | (1 << rng.integers(0, G, U)) | (1 << rng.integers(0, G, U)), m[:U])
        if kind == "zero":
            m[rng.choice(U, size=max(1, U // 50), replace=False)] = 0  # users outside every group
            m[0] = 0
    return dev(m)


@pytest.mark.parametrize("kind", MEMBERSHIPS)
@pytest.mark.parametrize("name", ["tiny", "small", "constructed"])
def test_grouped_product_vs_float64(ops, name, kind, golden_tiny, golden_small):
    U, n, graph, csr, plain, A64 = _graph_case(ops, name, golden_tiny, golden_small)
    if name == "constructed":
        assert csr.n_long == 1 and csr.n_chunks == 3 and plain.n_long == 0
    G = 3
    rng = _rng("grouped", name, kind)
    member = _membership(kind, U, n, G, rng)
    hot = ref.groups_of(member, G)  # [n, G]
    Xs, V, S_in = _randn(rng, (n, D)), _randn(rng, (n, D)), _randn(rng, (n, D))
    Xg = _randn(rng, (G, n, D))
    Xg_nan = torch.where(hot.t()[:, :, None], Xg, torch.full_like(Xg, NAN)).contiguous()  # NaN in every row that must not be read
    for grouped in (False, True):
        for with_v in (False, True):
            want = {}
            for nm, dtype in (("64", F64), ("32", F32)):
                A = A64.to(dtype)
                t = []
                for g in range(G):
                    x = (Xg[g] if grouped else Xs).to(dtype) + (V.to(dtype) if with_v else 0)
                    dg = hot[:, g:g + 1].to(dtype)
                    t.append(dg * (A @ (dg * x)))
                want[nm] = torch.stack(t)
            X = Xg_nan if grouped else Xs
            for outs in ("Y", "S", "YS", "YS+"):
                tag = "%s %s %s X%s %s" % (name, kind, "grouped" if grouped else "shared", " + V" if with_v else "", outs)
                Y = torch.full((G, n, D), NAN, device="cuda") if "Y" in outs else None
                S = torch.full((n, D), NAN, device="cuda") if "S" in outs else None
                sin = S_in if outs.endswith("+") else None
                ops.grouped_spmm_raw(csr, member, X, G, V=V if with_v else None, Y=Y, S=S, S_in=sin)
                if Y is not None:
                    written = hot.t()[:, :, None].expand(G, n, D)
                    assert torch.isnan(Y[~written]).all(), tag + ": a row outside its group was written"
                    assert torch.isfinite(Y[written]).all(), tag + ": NaN in a produced row"
                    _check(tag + " Y", torch.where(written, Y, torch.zeros_like(Y)), want["64"], want["32"], quiet=outs != "YS+")
                    if kind == "all" and not grouped:  # every group for everyone: each Y_g is the plain product
                        plain_y = ops.spmm(graph, Xs + V if with_v else Xs)
                        ref64 = A64 @ (Xs.double() + (V.double() if with_v else 0))
                        for g in range(G):
                            _check(tag + " Y_%d next to ops.spmm" % g, Y[g], ref64, plain_y, quiet=True)
                            _check(tag + " ops.spmm next to Y_%d" % g, plain_y, ref64, Y[g], quiet=True)
                if S is not None:
                    assert torch.isfinite(S).all(), tag
                    base = (lambda d: sin.to(d)) if sin is not None else (lambda d: 0)  # noqa: E731
                    _check(tag + " S", S, base(F64) + want["64"].sum(0), base(F32) + want["32"].sum(0), quiet=outs != "YS+")
                    if kind == "zero":  # a user outside every group receives nothing
                        outside = member == 0
                        assert torch.equal(S[outside], sin[outside] if sin is not None else torch.zeros_like(S[outside]))
                # the long-row schedule changes which wave sums a chunk, not the order of the sum
                Y2 = torch.full((G, n, D), NAN, device="cuda") if Y is not None else None
                S2 = torch.full((n, D), NAN, device="cuda") if S is not None else None
                ops.grouped_spmm_raw(plain, member, X, G, V=V if with_v else None, Y=Y2, S=S2, S_in=sin)
                for a, b in ((Y, Y2), (S, S2)):
                    assert a is None or torch.equal(a.view(torch.int32), b.view(torch.int32)), tag + ": bits depend on the schedule"


def test_grouped_product_live_row_bitmaps(ops, golden_tiny, golden_small):
    """x_rows / v_rows: rows whose bit is clear count as zero and are NOT read (they hold NaN here) — the first and the later
    products of the fused step's backward, whose input lives at the batch's rows only."""
    U, n, graph, csr, plain, A64 = _graph_case(ops, "small", golden_tiny, golden_small)
    G = 3
    rng = _rng("bitmaps")
    member = _membership("multi", U, n, G, rng)
    hot = ref.groups_of(member, G)
    live = np.sort(rng.choice(n, size=n // 5, replace=False))
    bits = _bitmap(n, live)
    flag = torch.zeros(n, dtype=torch.bool, device="cuda")
    flag[dev(live)] = True
    gF = _randn(rng, (n, D))
    gF_nan = torch.where(flag[:, None], gF, torch.full_like(gF, NAN))
    gF0 = torch.where(flag[:, None], gF, torch.zeros_like(gF))
    H = _randn(rng, (G, n, D))
    for nm, X, kw, x_of in (("x_rows", gF_nan, dict(x_rows=bits), lambda g, d: gF0.to(d)),
                            ("v_rows", H, dict(V=gF_nan, v_rows=bits), lambda g, d: H[g].to(d) + gF0.to(d))):
        want = {}
        for key, dtype in (("64", F64), ("32", F32)):
            dg = hot.to(dtype)
            want[key] = torch.stack([dg[:, g:g + 1] * (A64.to(dtype) @ (dg[:, g:g + 1] * x_of(g, dtype))) for g in range(G)])
        Y, S = torch.full((G, n, D), NAN, device="cuda"), torch.full((n, D), NAN, device="cuda")
        ops.grouped_spmm_raw(csr, member, X, G, Y=Y, S=S, **kw)
        written = hot.t()[:, :, None].expand(G, n, D)
        assert torch.isfinite(Y[written]).all() and torch.isfinite(S).all(), nm
        _check("small multi %s Y" % nm, torch.where(written, Y, torch.zeros_like(Y)), want["64"], want["32"])
        _check("small multi %s S" % nm, S, want["64"].sum(0), want["32"].sum(0))


# ======================================================================================================= (c) run to run
def test_two_runs_give_equal_bits(ops, golden_tiny, golden_small):
    rng = _rng("bits")
    n, G = 32833, 3
    ego, side = _randn(rng, (n, D), 0.1), _randn(rng, (n, D), 0.1)
    Wfc, bfc = _linear(rng, D, D)
    Wgrp, bgrp = _linear(rng, G, D)
    runs = []
    for _ in range(2):
        scores = torch.empty(n, G, device="cuda")
        member = ops.group_assign_raw(ego, side, Wfc, bfc, Wgrp, bgrp, n // 2, 0.4, SEED, 5, 9, scores_out=scores)
        runs.append((member.clone(), scores.view(torch.int32).clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    U, n, graph, csr, plain, A64 = _graph_case(ops, "constructed", golden_tiny, golden_small)
    member = _membership("multi", U, n, G, rng)
    X, V = _randn(rng, (G, n, D)), _randn(rng, (n, D))
    runs = []
    for _ in range(2):
        Y, S = torch.zeros((G, n, D), device="cuda"), torch.empty((n, D), device="cuda")
        ops.grouped_spmm_raw(csr, member, X, G, V=V, Y=Y, S=S)
        runs.append((Y.view(torch.int32).clone(), S.view(torch.int32).clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


# ============================================================================================ (d) the differentiable operator
def _propagate_setup(ops, golden_tiny, golden_small, d, L, G):
    U, n, graph, csr, plain, A64 = _graph_case(ops, "small", golden_tiny, golden_small)
    rng = _rng("propagate", d, L, G)
    member = _membership("multi", U, n, G, rng)
    E0 = _randn(rng, (n, d), 0.1)
    users, pos, neg = (dev(rng.integers(0, hi, 128).astype(np.int64)) for hi in (U, n - U, n - U))
    return U, n, csr, A64, member, E0, users, pos, neg


def test_autograd_at_width_64_is_the_raw_calls_bit_for_bit(ops, golden_tiny, golden_small):
    G, L = 3, 4
    U, n, csr, A64, member, E0, users, pos, neg = _propagate_setup(ops, golden_tiny, golden_small, D, L, G)
    leaf = E0.clone().requires_grad_(True)
    sums = ops.grouped_propagate(csr, leaf, member, L - 1, G)
    total = ops.grouped_propagate(csr, leaf, member, L - 1, G, summed=True)
    assert len(sums) == L - 1
    X, raw = E0, []
    for l in range(L - 1):
        Y, S = torch.zeros((G, n, D), device="cuda"), torch.empty((n, D), device="cuda")
        ops.grouped_spmm_raw(csr, member, X, G, Y=Y, S=S)
        raw.append(S)
        X = Y
    for a, b in zip(sums, raw):
        assert torch.equal(a.detach().view(torch.int32), b.view(torch.int32))
    acc = None
    X = E0
    for l in range(L - 1):
        Y = torch.zeros((G, n, D), device="cuda")
        acc = ops.grouped_spmm_raw(csr, member, X, G, Y=Y, S=torch.empty((n, D), device="cuda") if acc is None else acc, S_in=acc)[1]
        X = Y
    assert torch.equal(total.detach().view(torch.int32), acc.view(torch.int32))
    # the backward: the Horner chain through the same kernel
    g_out = _randn(_rng("gout"), (n, D))
    (got,) = torch.autograd.grad(total, leaf, g_out)
    H = None
    for l in range(L - 1, 0, -1):
        Y = torch.zeros((G, n, D), device="cuda") if l > 1 else None
        S = torch.empty((n, D), device="cuda") if l == 1 else None
        if H is None:
            ops.grouped_spmm_raw(csr, member, g_out, G, Y=Y, S=S)
        else:
            ops.grouped_spmm_raw(csr, member, H, G, V=g_out, Y=Y, S=S)
        H = Y
    assert torch.equal(got.view(torch.int32), S.view(torch.int32))


@pytest.mark.parametrize("d", [64, 128])
def test_autograd_vs_step64(ops, d, golden_tiny, golden_small):
    """final = (G E0 + sum_l S_l) / L under autograd, fed d loss / d final of step64: the ego gradient of the whole step.
    d = 128 runs the composition (row masks in torch around ops.spmm)."""
    G, L = 3, 4
    U, n, csr, A64, member, E0, users, pos, neg = _propagate_setup(ops, golden_tiny, golden_small, d, L, G)
    want = {k: ref.step64(A64, E0, member, users, pos, neg, G, L, REG, U, dtype=dt) for k, dt in (("64", F64), ("32", F32))}
    leaf = E0.clone().requires_grad_(True)
    final = (G * leaf + ops.grouped_propagate(csr, leaf, member, L - 1, G, summed=True)) / L
    _check("autograd d=%d final" % d, final.detach(), want["64"][2], want["32"][2])
    (g,) = torch.autograd.grad(final, leaf, want["32"][3])
    _, _, ge64 = ref.bpr64(want["64"][2], E0, U, users, pos, neg, REG, reg_users=True)  # the regulariser's rows
    _check("autograd d=%d d E0" % d, g.double() + ge64, want["64"][1], want["32"][1])
    lists = ops.grouped_propagate(csr, leaf, member, L - 1, G)
    _check("autograd d=%d list form" % d, sum(t.detach() for t in lists), want["64"][2] * L - G * E0.double(), want["32"][2] * L - G * E0)


# ================================================================================================================ (e) the engine
ENGINE_CASES = [(3, 6, 0.0), (3, 6, 0.4), (2, 3, 0.0), (2, 3, 0.4), (3, 1, 0.0), (3, 1, 0.4)]
_engine_runs = {}


def _engine_run(ops, golden_tiny, golden_small, golden_impgcn, G, L, p):
    key = (G, L, p)
    if key in _engine_runs:
        return _engine_runs[key]
    from idgrec_amd.impgcn import ImpgcnEngine

    U, n, graph, csr, plain, A64 = _graph_case(ops, "small", golden_tiny, golden_small)
    rng = _rng("engine", *key)
    xav = lambda r, c: dev(rng.uniform(-np.sqrt(6.0 / (r + c)), np.sqrt(6.0 / (r + c)), (r, c)).astype(np.float32))  # noqa: E731
    P0 = torch.cat([xav(U, D), xav(n - U, D)])
    small0 = _linear(rng, D, D) + _linear(rng, G, D)
    batches = [tuple(dev(golden_impgcn["batch"][:, c]) for c in range(3)),
               tuple(dev(golden_impgcn["traj_batches"][256:512, c]) for c in range(3))]  # ([:256] contains the B = 96 batch)
    eng = ImpgcnEngine(graph, csr, U, n - U, P0.clone(), small0, L, p=p, reg_lambda=REG, lr=LR, store_grad=True)
    SW0 = eng.SW.clone()
    steps = []
    for s, (users, pos, neg) in enumerate(batches):
        streams = ((SEED + s, 5), (SEED + s, 9))
        P_before = eng.P.clone()
        loss = eng.train_step(users, pos, neg, streams=streams).clone()
        st = dict(loss=loss, GRAD=eng.GRAD.clone(), P=eng.P.clone(), M=eng.M.clone(), V=eng.V.clone(), final=eng.FINAL.clone(),
                  member=eng.member.clone(), SW=eng.SW.clone(), SM=eng.SM.clone(), SV=eng.SV.clone())
        m1 = None if p == 0 else ref.keep_mask(p, SEED + s, 5, n, D).cuda()
        m2 = None if p == 0 else ref.keep_mask(p, SEED + s, 9, n, G).cuda()
        st["assign"] = ref.assign64(P_before, A64 @ P_before.double(), *small0, U, m1, m2)
        for name, dtype in (("64", F64), ("32", F32)):  # fed the DEVICE's membership
            st["loss" + name], st["GRAD" + name], st["final" + name], _ = ref.step64(A64, P_before, st["member"], users, pos, neg, G, L,
                                                                                    REG, U, dtype=dtype)
        steps.append(st)
    eval_final = eng.forward(training=False).clone()
    eval_member = eng.member.clone()
    run = dict(P0=P0, SW0=SW0, steps=steps, eval=(eval_final, eval_member, eng.P.clone()), small0=small0, A64=A64, U=U)
    torch.cuda.synchronize()
    _engine_runs[key] = run
    return run


@pytest.mark.parametrize("G,L,p", ENGINE_CASES)
def test_engine_two_steps_vs_float64(ops, G, L, p, golden_tiny, golden_small, golden_impgcn):
    """The second step's batch names other rows than the first's: rows of step 1 leaking into step 2 — through GFIN, which the
    backward's products read at the batch's rows only, through the regulariser's panel, through the bitmap — would show in
    its table gradient.  No dense panel is zeroed between the steps."""
    run = _engine_run(ops, golden_tiny, golden_small, golden_impgcn, G, L, p)
    U = run["U"]
    for s, st in enumerate(run["steps"], 1):
        tag = "engine G=%d L=%d p=%g step %d" % (G, L, p, s)
        _, member64, near = st["assign"]
        assert int(near.sum()) <= 0.005 * member64.shape[0]
        assert bool(((st["member"] == member64) | near).all()), tag + ": membership"
        assert (st["member"][U:] == (1 << G) - 1).all()
        if p > 0 and G > 1:
            assert int(((st["member"][:U] & (st["member"][:U] - 1)) != 0).sum()) > 0  # ties happen
        assert torch.isfinite(st["loss"]).all() and torch.isfinite(st["GRAD"]).all()
        for k, name in enumerate(("bpr", "reg")):
            _check("%s loss %s" % (tag, name), st["loss"][k], st["loss64"][k], st["loss32"][k])
        _check(tag + " final", st["final"], st["final64"], st["final32"])
        _check(tag + " GRAD", st["GRAD"], st["GRAD64"], st["GRAD32"])
        assert torch.equal(st["GRAD"].abs().sum(dim=1) == 0, st["GRAD64"].abs().sum(dim=1) == 0), tag + ": other rows receive gradient"
        # the four small tensors: bit-unchanged, zero moments
        assert torch.equal(st["SW"].view(torch.int32), run["SW0"].view(torch.int32)), tag
        assert not st["SM"].any() and not st["SV"].any(), tag
    # Adam (tests/test_gpu_gccf.py's rule): moments within 4 * 2^-24 of their largest entry, the table within 4 ulp of its own
    want = ref.adam64(run["P0"], [st["GRAD"] for st in run["steps"]], lr=LR)
    for s, (st, (W, M, V)) in enumerate(zip(run["steps"], want), 1):
        for name, got, w in (("exp_avg", st["M"], M), ("exp_avg_sq", st["V"], V)):
            e = float((got.double() - w).abs().max() / w.abs().max())
            print("  G=%d L=%d p=%g step %d %s: %.2f * 2^-24 of max" % (G, L, p, s, name, e * 2.0 ** 24))
            assert e <= 4 * 2.0 ** -24, (name, s, e)
        ulp = float(np.spacing(np.float32(float(W.abs().max()))))
        e = float((st["P"].double() - W).abs().max())
        print("  G=%d L=%d p=%g step %d table: %.2f ulp of max" % (G, L, p, s, e / ulp))
        assert e <= 4 * ulp, (s, e / ulp)
    assert not torch.equal(run["steps"][0]["P"], run["steps"][1]["P"])
    # evaluation panels: dropout off
    eval_final, eval_member, P_now = run["eval"]
    _, member64, near = ref.assign64(P_now, run["A64"] @ P_now.double(), *run["small0"], U)
    assert bool(((eval_member == member64) | near).all()) and int(near.sum()) <= 0.005 * member64.shape[0]
    assert int(((eval_member[:U] & (eval_member[:U] - 1)) != 0).sum()) == 0
    _check("engine G=%d L=%d p=%g evaluation panels" % (G, L, p), eval_final, ref.final64(run["A64"], P_now, eval_member, G, L),
           ref.final64(run["A64"], P_now, eval_member, G, L, dtype=F32))


# ================================================================================================================ (f) the plugin
def _cfg(**kw):
    import utility.utility_function.tools as tools

    cfg = tools.read_configuration(os.path.join(ROOT, "configure", "IMPGCN.txt"), "IMPGCN")
    cfg.update({k: str(v) for k, v in kw.items()})
    return cfg


def _data(tmp_path, g, name, cfg):
    import utility.utility_data.data_loader as data_loader

    d = tmp_path / name
    d.mkdir(exist_ok=True)
    (d / "train.txt").write_bytes(g["train_txt"].tobytes())
    (d / "test.txt").write_bytes(g["test_txt"].tobytes())
    cfg.update(dataset=name, dataset_path=str(tmp_path) + "/", sparsity_test="0")
    return data_loader.Data(str(d), cfg)


def _model(ops, tmp_path, golden_small, **extra):
    import utility.utility_function.tools as tools
    from models.IMPGCN import IMPGCN

    cfg = _cfg(**extra)
    data = _data(tmp_path, golden_small, "small", cfg)
    tools.set_seed(2024)
    return IMPGCN(cfg, data, torch.device("cuda")).to("cuda"), cfg, data


@pytest.mark.parametrize("tag,G,L", [("def", 3, 6), ("two", 2, 3)])
def test_model_matches_reference_goldens(ops, tag, G, L, tmp_path, golden_small, golden_impgcn):
    g = golden_impgcn
    m, cfg, data = _model(ops, tmp_path, golden_small, group=G, GCN_layer=L)
    U = data.num_users
    cpu = lambda t: t.detach().cpu().numpy()  # noqa: E731
    # same torch RNG order as the reference's constructor
    assert np.array_equal(cpu(m.user_embedding.weight), g["init_user"]) and np.array_equal(cpu(m.item_embedding.weight), g["init_item"])
    assert np.array_equal(cpu(m.fc.weight), g["fc_weight"]) and np.array_equal(cpu(m.fc.bias), g["fc_bias"])
    assert np.array_equal(cpu(m.fc_group.weight), g[tag + "_fc_group_weight"]) and np.array_equal(cpu(m.fc_group.bias), g[tag + "_fc_group_bias"])
    assert len(list(m.parameters())) == 6
    # evaluation: membership, panels, rating
    m.eval()
    assert np.array_equal(cpu(m.membership(m.ego_panel(), False)), g[tag + "_eval_member"])
    ue, ie = m.final_panels()
    np.testing.assert_allclose(cpu(ue), g[tag + "_eval_user"], rtol=1e-4, atol=1e-7)
    np.testing.assert_allclose(cpu(ie), g[tag + "_eval_item"], rtol=1e-4, atol=1e-7)
    au, ai = m.aggregate()
    np.testing.assert_allclose(cpu(au), g[tag + "_eval_user"], rtol=1e-4, atol=1e-7)
    users = torch.from_numpy(g["rating_users"]).cuda()
    np.testing.assert_allclose(cpu(m.get_rating_for_test(users)), g[tag + "_rating"], rtol=1e-4, atol=1e-5)
    assert m.topk_for_test(users, 10).shape == (32, 10)
    # training under the published masks: the device seed and the stream counter are the golden's
    m.train()
    torch.cuda.manual_seed(int(g["mask_seed"]))
    ops.reset_noise_stream(int(g["grad_streams"][0]) - 1)
    b = torch.from_numpy(g["batch"]).cuda()
    m.zero_grad()
    ll = m(b[:, 0], b[:, 1], b[:, 2])
    assert len(ll) == 2
    print("losses", [x.item() for x in ll], g[tag + "_loss"])
    np.testing.assert_allclose([x.item() for x in ll], g[tag + "_loss"], rtol=1e-4)
    sum(ll).backward()
    np.testing.assert_allclose(cpu(m.user_embedding.weight.grad), g[tag + "_grad_user"], rtol=1e-3, atol=1e-8)
    np.testing.assert_allclose(cpu(m.item_embedding.weight.grad), g[tag + "_grad_item"], rtol=1e-3, atol=1e-8)
    assert all(prm.grad is None for prm in (m.fc.weight, m.fc.bias, m.fc_group.weight, m.fc_group.bias))  # as in the reference
    ops.reset_noise_stream(int(g["grad_streams"][0]) - 1)
    assert np.array_equal(cpu(m.membership(m.ego_panel(), True)), g[tag + "_member"])
    # three fused steps against the reference's own Adam trajectory
    tri = torch.from_numpy(g["traj_batches"]).cuda()
    m, cfg, data = _model(ops, tmp_path, golden_small, group=G, GCN_layer=L)
    assert m.fused_step_available()
    torch.cuda.manual_seed(int(g["mask_seed"]))
    ops.reset_noise_stream(int(g["traj_streams"][0, 0]) - 1)
    opt = ops.Adam(m.parameters(), lr=float(cfg["learn_rate"]))
    loss = torch.zeros((3, 2), device="cuda")
    small0 = [prm.detach().clone() for prm in list(m.parameters())[2:]]
    for i in range(3):
        bt = tuple(tri[i * 256:(i + 1) * 256, c].contiguous() for c in range(3))
        m.prefetch_batch(*bt)
        assert m.fused_train_step(*bt, loss[i], opt)
        assert np.array_equal(cpu(m.impgcn_engine().member), g[tag + "_traj_member"][i]), i
    print("trajectory losses", loss.cpu().numpy(), g[tag + "_traj_loss"])
    np.testing.assert_allclose(loss.cpu().numpy(), g[tag + "_traj_loss"], rtol=1e-5)
    for mine, want in ((m.user_embedding.weight, g[tag + "_traj_user"]), (m.item_embedding.weight, g[tag + "_traj_item"])):
        mine = cpu(mine)
        off = ~np.isclose(mine, want, rtol=1e-4, atol=1e-6)
        print("trajectory: off %.3g, max %.3g" % (off.mean(), np.abs(mine - want).max()))
        assert off.mean() < 1e-3, off.mean()
        assert np.abs(mine - want).max() < 1e-4, np.abs(mine - want).max()
    for prm, was in zip(list(m.parameters())[2:], small0):  # fc / fc_group keep their initial values, as in the reference
        assert torch.equal(prm.detach(), was)
    assert all(int(opt.state[prm]["step"]) == 3 for prm in m.parameters())


def test_model_path_that_does_not_fuse(ops, tmp_path, golden_small):
    """embedding_size = 128: the composition only; finite losses, a gradient for both tables, none for fc / fc_group."""
    m, cfg, data = _model(ops, tmp_path, golden_small, embedding_size=128)
    assert not m.fused_step_available()
    rng = _rng("batch")
    b = [dev(rng.integers(0, hi, 128).astype(np.int64)) for hi in (300, 250, 250)]
    m.train()
    ll = m(*b)
    sum(ll).backward()
    assert all(torch.isfinite(x).all() for x in ll)
    for prm in (m.user_embedding.weight, m.item_embedding.weight):
        assert prm.grad is not None and torch.isfinite(prm.grad).all() and float(prm.grad.abs().max()) > 0
    assert m.fc.weight.grad is None and m.fc_group.bias.grad is None
    m.eval()
    assert m.get_rating_for_test(b[0][:8]).shape == (8, 250)


# ============================================================================================================= (g) the hand-off
def _handoff_model(ops, tmp_path, g, golden_impgcn):
    m, cfg, data = _model(ops, tmp_path, g)
    assert m.fused_step_available()
    params = list(m.parameters())
    assert len(params) == 6
    tri = torch.from_numpy(golden_impgcn["traj_batches"]).cuda()
    batches = [tuple(tri[i * 256:(i + 1) * 256, c].contiguous() for c in range(3)) for i in range(3)]
    return m, params, batches, torch.zeros(m.n_fused_losses, device="cuda")


def _inside(t, buffers):
    lo, hi = t.data_ptr(), t.data_ptr() + 4 * t.numel()
    return any(b.data_ptr() <= lo and hi <= b.data_ptr() + 4 * b.numel() for b in buffers)


def test_adam_state_hand_off(ops, tmp_path, golden_small, golden_impgcn):
    """tests/test_gpu_engine_handoff.py's three cases: a foreign optimizer is refused and nothing moves; an optimizer that has
    stepped the other way keeps what it accumulated (the four small tensors: a ZERO gradient from fused_loss_and_grad, hence
    zero moments and an unchanged value, and a step counter that agrees); disagreeing counters are refused."""
    m, params, batches, loss = _handoff_model(ops, tmp_path, golden_small, golden_impgcn)
    eng = m._fused_engine()
    opt = torch.optim.Adam(params, lr=1e-3)
    held = [eng.M, eng.V, eng.SM, eng.SV]
    before = [t.detach().clone() for t in params + held]
    assert m.fused_train_step(*batches[0], loss, opt) is False and m._engine_adam(opt) is None
    torch.cuda.synchronize()
    assert all(torch.equal(t.detach(), was) for t, was in zip(params + held, before)) and not opt.state
    # stepped the other way
    m, params, batches, loss = _handoff_model(ops, tmp_path, golden_small, golden_impgcn)
    small0 = [p.detach().clone() for p in params[2:]]
    opt = ops.Adam(params, lr=1e-3)
    m.fused_loss_and_grad(*batches[0])
    opt.step()
    want = [(opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for p in params]
    assert all(int(opt.state[p]["step"]) == 1 for p in params)
    adam = m._engine_adam(opt)
    assert adam is not None and adam[0] is opt.param_groups[0] and adam[1] == 1
    eng = m._fused_engine()
    for k, (p, (wm, wv)) in enumerate(zip(params, want)):
        st = opt.state[p]
        assert torch.equal(st["exp_avg"], wm) and torch.equal(st["exp_avg_sq"], wv)
        assert (float(wm.abs().max()) > 0) == (k < 2)
        assert _inside(st["exp_avg"], [eng.M, eng.SM]) and _inside(st["exp_avg_sq"], [eng.V, eng.SV])
    for b in batches[1:]:
        assert m.fused_train_step(*b, loss, opt) is True and torch.isfinite(loss).all()
    assert m._fused_engine() is eng and all(int(opt.state[p]["step"]) == 3 for p in params)
    assert all(torch.isfinite(p.detach()).all() for p in params)
    assert all(torch.equal(p.detach(), was) for p, was in zip(params[2:], small0)) and not eng.SM.any() and not eng.SV.any()
    # disagreeing counters
    opt.state[params[-1]]["step"] += 1
    before = [p.detach().clone() for p in params]
    assert m.fused_train_step(*batches[0], loss, opt) is False and m._engine_adam(opt) is None
    torch.cuda.synchronize()
    assert all(torch.equal(p.detach(), was) for p, was in zip(params, before))
    assert [int(opt.state[p]["step"]) for p in params] == [3] * 5 + [4]
