"""idg_bpr.hip — the BPR forward (bpr_triple_kernel), the sorted and the atomic scatter, the three sorting routes of the
scatter plan, the loss reduction and both Adam kernels — against float64, across their dispatch.  The reference statement
is tests/bpr_ref64.py, pinned to the reference's own numbers by tests/test_bpr_ref.py.

  (a) the plain form (ops.bpr_fused_raw, ops.bpr_loss) at every width class and batch edge, deterministic and atomic;
  (b) MFBPR: one panel receiving both gradients;
  (c) idg_bpr_fused_ex_f32 through ctypes: final and ego rows of different widths, item-only regulariser;
  (d) saturated sigmoids next to the 1e-7 guard;
  (e) the sort routes of bpr_sort_plan with 32- and 64-bit packed keys: the plan itself, then the scatter consuming it;
  (f) upstream scalars other than (1, 1);
  (g) idg_adam_step_f32 and idg_adam_rows_f32.

One tolerance rule throughout (egcf_ref64.errors / band): with scale = max |ref64| of the tensor compared,
    e_kernel = max |kernel - ref64| / scale   <=   max(4 e_f32, 8 * 2^-24),   e_f32 = max |float32 composition - ref64| / scale
where the float32 composition is bpr_ref64's same expressions in float32, run in the same test; both numbers are printed
(pytest -s).  It is applied to each gradient panel on its own scale and to each of the two losses on the scale |ref64 loss|.
Argued rather than met: the rows that 64 or more slots name, in _Case.check only — see _Case._check_panel.
The one case with NO scale — d total / d final under upstream (0, 1), identically zero — is asserted to be exactly zero.

Bit claims (torch.equal) where the code makes them: run to run, planned versus sorted in the call, bitmap store versus
accumulation into zeros, preset bitmap versus bits set by the scatter, forward + backward with upstream (1, 1) versus the
fused call, the rider block's loss versus the stand-alone reduction, row-Adam with all / no bits versus the flat step.

Measured on an MI355X (146 tests, 7.3 .. 7.9 s for the whole file), e_kernel / e_f32 on the plain scale, worst e_kernel / band:
  (a) gradients 0 .. 3.3e-7 / 0 .. 3.4e-7 (0.56), losses 1e-10 .. 8.6e-7 / the same (0.52)
  (b) gradients 3.6e-9 .. 1.9e-7 / 4.2e-9 .. 1.6e-7 (0.40), losses 2.3e-9 .. 8.9e-8 (0.19)
  (c) gradients 6.8e-10 .. 2.3e-7 / 6.0e-10 .. 1.8e-7 (0.49), losses 6.7e-10 .. 2.2e-7 / 2.4e-9 .. 1.7e-7 (0.47)
  (d) gradients 7.1e-8 .. 2.0e-6 / 7.1e-8 .. 1.6e-6 (0.31), losses 9.1e-8 .. 1.9e-7 (0.25)
  (e) gradients 1.2e-7 .. 8.6e-7 / the same (0.51), losses 1.5e-8 .. 1.7e-7 / 1.5e-8 .. 8.2e-8 (0.35)
  (f) gradients 1.2e-7 .. 3.3e-6 / 3.8e-7 .. 2.1e-6 (0.42), losses 3.3e-8 .. 1.5e-7 (0.25)
  (g) moments and table change 2.5e-16 .. 2.7e-5 / the same (0.25)
  rows of >= 64 slots (168 checks in (a) - (c)): e_kernel up to 7.9e-6 (one-panel MFBPR, hub, atomic, d = 20) against the
  argued floor 1.6e-5; under the plain floor six of them missed, by 1.001x to 3.4x (see _Case._check_panel).
Value-only breaks of a scratch copy of the library, one run of this file each, made while the long rows still had the
plain floor; tests failing IN ADDITION to the six that missed that floor: the scatter's `reg += r1` loop dropped 61 (across
(a) - (f)); its twin in the `de` column loop 10 (the width-changing cases of (c)); `c * u` for negatives 76; the user ego
row read with reg_users == 0 6 (the item-only cases of (c)); `G` loaded regardless of `live` 24 (every test of
idg_adam_rows_f32 but the refusals)."""
import ctypes as C
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import bpr_ref64 as ref  # noqa: E402

F32, F64 = torch.float32, torch.float64
U0, I0 = 300, 200
REG = 1e-2
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    import idgrec_amd.ops as ops_

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return ops_


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _check(what, got, ref64, f32, scale=None):
    e_k, e_f = ref.errors(got, ref64, f32, scale)
    print("  %-66s e_kernel %.2e  e_f32 %.2e" % (what, e_k, e_f))
    assert e_k <= ref.band(e_f), "%s: e_kernel %.3e above max(4 e_f32 = %.3e, %.3e)" % (what, e_k, 4 * e_f, ref.FLOOR)
    return e_k, e_f


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _flags(bitmap, n):
    """bool [n] on the device: the bits of an int32 bitmap tensor."""
    idx = torch.arange(n, device=bitmap.device)
    return ((bitmap[idx >> 5] >> (idx & 31).int()) & 1).bool()


# ===================================================================================================== id-list patterns
def _ids(pattern, B, U, I, rng):
    users, pos, neg = rng.integers(0, U, B), rng.integers(0, I, B), rng.integers(0, I, B)
    if pattern == "random":
        pass
    elif pattern == "distinct":  # no row twice in a list; where the items suffice, no item row twice at all
        assert B <= I
        users = rng.choice(U, B, replace=False)
        if 2 * B <= I:
            both = rng.choice(I, 2 * B, replace=False)
            pos, neg = both[:B], both[B:]
        else:
            pos = rng.choice(I, B, replace=False)
            neg = np.roll(pos, 1) if B > 1 else (pos + 1) % I
    elif pattern == "hub":  # one item on 70 positions as pos and 200 as neg (a run of 270 slots of both signs), one user on 130
        assert B >= 200
        h, hu = int(rng.integers(0, I)), int(rng.integers(0, U))
        pos[rng.choice(B, 70, replace=False)] = h
        neg[rng.choice(B, 200, replace=False)] = h
        users[rng.choice(B, 130, replace=False)] = hu
    elif pattern == "same":
        users[:], pos[:] = users[0], pos[0]
        neg[:] = neg[0] if neg[0] != pos[0] else (pos[0] + 1) % I
    elif pattern == "selfpair":  # pos[i] == neg[i] on a quarter of the triples
        assert B >= 3
        q = rng.choice(B, max(1, B // 4), replace=False)
        neg[q] = pos[q]
    else:
        assert pattern == "edges" and B >= 2  # rows 0, U - 1, U and n - 1, each as more than one role
        users[0], users[1] = 0, U - 1
        pos[0], neg[0] = 0, I - 1
        pos[1], neg[1] = I - 1, 0
    return users.astype(np.int64), pos.astype(np.int64), neg.astype(np.int64)


def _patterns(B):
    if B == 1:
        return ["random"]
    pats = ["random", "distinct", "same", "selfpair", "edges"]
    return pats + ["hub"] if B >= 200 else pats


class _Case:
    """Panels (0.3 * randn), id lists and the float64 / float32 statements of one case."""

    def __init__(self, key, d, B, pattern, de=None, reg_users=True, same=False, U=U0, I=I0, upstream=None, ids=None):
        rng = np.random.default_rng(_seed(key, d, B, pattern, de, reg_users, same))
        self.d, self.de, self.B, self.U, self.I, self.n = d, (d if de is None else de), B, U, I, U + I
        self.reg_users, self.same, self.upstream = reg_users, same, upstream
        self.tag = "%s d=%d%s B=%d %s%s" % (key, d, "" if de is None else "/%d" % de, B, pattern, "" if reg_users else " items-only")
        users, pos, neg = _ids(pattern, B, U, I, rng) if ids is None else ids
        self.ids_np = (users, pos, neg)
        self.users, self.pos, self.neg = dev(users), dev(pos), dev(neg)
        self.rows = torch.unique(torch.cat([self.users, U + self.pos, U + self.neg]))
        self.fin_np = (0.3 * rng.standard_normal((self.n, d))).astype(np.float32)
        self.ego_np = None if same else (0.3 * rng.standard_normal((self.n, self.de))).astype(np.float32)
        self._ref = None

    def upload(self):
        self.fin = dev(self.fin_np)
        self.ego = self.fin if self.same else dev(self.ego_np)
        return self

    def refs(self):
        if self._ref is None:
            a = (self.fin, self.ego, self.U, self.users, self.pos, self.neg, REG)
            self._ref = (ref.bpr64(*a, reg_users=self.reg_users, dtype=F64, upstream=self.upstream),
                         ref.bpr64(*a, reg_users=self.reg_users, dtype=F32, upstream=self.upstream))
        return self._ref

    def check(self, what, loss, gf, ge):
        (l64, gf64, ge64), (l32, gf32, ge32) = self.refs()
        tag = self.tag + " " + what
        if loss is not None:
            for k in range(2):
                _check("%s loss[%d]" % (tag, k), loss[k], l64[k], l32[k])
        assert torch.isfinite(gf).all() and torch.isfinite(ge).all()
        self._check_panel(tag + (" g (one panel)" if self.same else " g_final"), gf, gf64, gf32)
        if not self.same:
            self._check_panel(tag + " g_ego", ge, ge64, ge32)

    def _check_panel(self, what, got, r64, r32):
        """The rule on the scale max |ref64| of the whole panel.  Rows that m >= 64 slots name (only `same` at B >= 64 and
        `hub` have any: runs of 64, 131, 200 and 271) are held to  max(4 e_f32, (m - 1) 2^-24)  on that same scale: the
        kernels add a row's m terms one after the other (the atomic scatter in any order) and recursive summation may
        sit (m - 1) 2^-24 sum |t_i| from the exact sum, while the float32 composition's scatter adds pairwise and does
        not grow with m.  Measured with the plain floor on those rows: six misses, all there, at 1.0 to 3.4 times the
        band (e_kernel 8.8e-7 .. 7.1e-6; the argued floor is 3.8e-6 at m = 64, 1.6e-5 at m = 271).  Every other row of
        every case keeps the plain rule."""
        scale = float(r64.abs().max())
        m = torch.bincount(torch.cat([self.users, self.U + self.pos, self.U + self.neg]), minlength=self.n)
        long = m >= 64
        _check(what, got[~long], r64[~long], r32[~long], scale)
        if long.any():
            e_k, e_f = ref.errors(got[long], r64[long], r32[long], scale)
            floor = (int(m.max()) - 1) * 2.0 ** -24
            print("  %-66s e_kernel %.2e  e_f32 %.2e  (rows of >= 64 slots, floor %.2e)" % (what, e_k, e_f, floor))
            assert e_k <= max(4 * e_f, floor), "%s, rows of >= 64 slots: e_kernel %.3e above max(4 e_f32 = %.3e, %.3e)" % (
                what, e_k, 4 * e_f, floor)


def _run(ops, c, det=1, mode="acc", planned=False, ex=False, prefill_ego_users=None):
    """One fused call.  mode: "acc" accumulates into zero-filled panels; "store" hands a zeroed bitmap and NaN-filled panels;
    "preset" the same with the bitmap filled by bpr_touch_rows_raw and IDG_BPR_TOUCHED_PRESET.  ex: idg_bpr_fused_ex_f32
    through ctypes (always when the widths differ or the regulariser is item-only).  Returns (loss, g_final, g_ego, bitmap)."""
    from idgrec_amd import native

    ex = ex or c.de != c.d or not c.reg_users
    ws = ops.bpr_workspace(c.B, c.d, "cuda")
    if planned:
        ops.bpr_plan_raw(c.users, c.pos, c.neg, c.U, c.n, c.d, ws=ws)
        det = native.IDG_BPR_PLANNED
    fill = 0.0 if mode == "acc" else NAN
    gf = torch.full((c.n, c.d), fill, device="cuda")
    ge = gf if c.same else torch.full((c.n, c.de), fill, device="cuda")
    if prefill_ego_users is not None:
        ge[:c.U] = prefill_ego_users
    touched = None
    if mode != "acc":
        touched = torch.zeros((c.n + 31) // 32, dtype=torch.int32, device="cuda")
        if mode == "preset":
            ops.bpr_touch_rows_raw(c.users, c.pos, c.neg, c.U, touched)
            det = int(det) | native.IDG_BPR_TOUCHED_PRESET
    loss = torch.full((2,), NAN, device="cuda")
    if ex:
        native.check(native.lib.idg_bpr_fused_ex_f32(_p(c.fin), c.d, _p(c.ego), c.de, c.U, c.n, _p(c.users), _p(c.pos), _p(c.neg),
                                                     c.B, REG, int(c.reg_users), _p(loss), _p(gf), _p(ge), int(det), _p(touched),
                                                     _p(ws), ops._stream()), "idg_bpr_fused_ex_f32")
    else:
        ops.bpr_fused_raw(c.fin, c.ego, c.users, c.pos, c.neg, c.U, REG, gf, ge, loss=loss, deterministic=int(det),
                          touched=touched, ws=ws)
    return loss, gf, ge, touched


def _same_bits(a, b, what):
    assert torch.equal(a[0], b[0]), what + ": the loss has other bits"
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), what + ": a gradient panel has other bits"


def _bitmap_claims(ops, c, acc, ex=False):
    """Store mode against `acc` (the in-call sorted accumulation into zeros): the bitmap holds exactly the batch's rows, the
    flagged rows carry the same bits, every other row still holds its NaN prefill; the preset flag after bpr_touch_rows_raw
    (sorted in the call, and planned) gives what the scatter's own bits give."""
    want = torch.zeros(c.n, dtype=torch.bool, device="cuda")
    want[c.rows] = True
    for mode, planned in (("store", False), ("store", True), ("preset", False), ("preset", True)):
        what = "%s %s%s" % (c.tag, mode, " planned" if planned else "")
        loss, gf, ge, bm = _run(ops, c, mode=mode, planned=planned, ex=ex)
        fl = _flags(bm, c.n)
        assert torch.equal(fl, want), what + ": the bitmap is not the batch's row set"
        assert torch.equal(loss, acc[0]), what + ": loss bits"
        assert torch.equal(gf[fl], acc[1][fl]) and torch.equal(ge[fl], acc[2][fl]), what + ": stored rows differ from accumulated ones"
        assert torch.isnan(gf[~fl]).all() and torch.isnan(ge[~fl]).all(), what + ": a row outside the batch was written"


# ============================================================================================================ (a) plain form
WIDTHS = [1, 4, 20, 63, 64, 65, 100, 128, 256]  # below a wave; the `live = f < d` tail; exactly one pass; the f0 += WAVE loop


@pytest.mark.parametrize("B", [1, 3, 5, 64, 200])
@pytest.mark.parametrize("d", WIDTHS)
def test_plain_form_vs_float64(ops, d, B):
    """bpr_triple_kernel's one-width branch (de == d, reg_users) with its lane tail (d % 64 != 0) and second pass (d > 64);
    bpr_scatter_kernel's `live` tail, `f0 += WAVE` loop and, on `hub`, its `base += WAVE` loop over runs of 130 and 270
    slots at EVERY width; bpr_atomic_kernel; B = 1 and B not a multiple of the 4 waves of a workgroup (1, 3, 5: the
    `i >= B` / `j >= 3B` exits); rows 0, U - 1, U, n - 1 (`edges`); pos[i] == neg[i] (`selfpair`).  Deterministic:
    tolerance, run to run, planned == in-call, forward + backward through autograd (device upstream (1, 1), stand-alone
    1024-thread reduction) == the fused call with the rider block.  Atomic: tolerance only."""
    for pattern in _patterns(B):
        c = _Case("plain", d, B, pattern).upload()
        det = _run(ops, c)
        c.check("sorted", *det[:3])
        _same_bits(det, _run(ops, c), c.tag + " run to run")
        _same_bits(det, _run(ops, c, planned=True), c.tag + " planned")
        c.check("atomic", *_run(ops, c, det=0)[:3])
        rest = torch.ones(c.n, dtype=torch.bool, device="cuda")
        rest[c.rows] = False
        assert (det[1][rest] == 0).all() and (det[2][rest] == 0).all(), "a row named by no id list was written"
        f, e = c.fin.clone().requires_grad_(True), c.ego.clone().requires_grad_(True)
        bpr, reg = ops.bpr_loss(f, e, c.users, c.pos, c.neg, c.U, REG, True)
        (bpr + reg).backward()
        _same_bits(det, (torch.stack([bpr.detach(), reg.detach()]), f.grad, e.grad), c.tag + " autograd route")
        if pattern in ("random", "hub"):
            f, e = c.fin.clone().requires_grad_(True), c.ego.clone().requires_grad_(True)
            bpr, reg = ops.bpr_loss(f, e, c.users, c.pos, c.neg, c.U, REG, False)
            (bpr + reg).backward()
            c.check("autograd atomic", torch.stack([bpr.detach(), reg.detach()]), f.grad, e.grad)


@pytest.mark.parametrize("B", [5, 200])
@pytest.mark.parametrize("d", [20, 64, 100])
def test_plain_form_bitmap_store_and_preset(ops, d, B):
    """The touched bitmap of bpr_scatter_kernel (`a.touched`: rows stored, not accumulated; bits set by lane 0) and
    IDG_BPR_TOUCHED_PRESET outside an engine (bits set by bpr_touch_rows_raw beforehand, none written by the scatter)."""
    for pattern in _patterns(B):
        c = _Case("bitmap", d, B, pattern).upload()
        acc = _run(ops, c)
        c.check("sorted", *acc[:3])
        _bitmap_claims(ops, c, acc)


def test_plain_form_refuses_a_bitmap_with_the_atomic_scatter(ops):
    from idgrec_amd import native

    c = _Case("refuse", 64, 5, "random").upload()
    with pytest.raises(native.IdgError):
        _run(ops, c, det=0, mode="store")


# ================================================================================================================== (b) MFBPR
@pytest.mark.parametrize("pattern", ["hub", "selfpair"])
@pytest.mark.parametrize("d", [20, 64, 100])
def test_mfbpr_one_panel_vs_float64(ops, d, pattern):
    """g_final is g_ego (bpr_scatter_kernel's `a.g_final == a.g_ego` branch: acc + reg into one row, added or — with a
    bitmap — stored), sorted and atomic, and through ops.bpr_loss with one tensor passed twice."""
    c = _Case("mfbpr", d, 200, pattern, same=True).upload()
    det = _run(ops, c)
    assert det[1] is det[2]
    c.check("sorted", *det[:3])
    _same_bits(det, _run(ops, c), c.tag + " run to run")
    _same_bits(det, _run(ops, c, planned=True), c.tag + " planned")
    c.check("atomic", *_run(ops, c, det=0)[:3])
    _bitmap_claims(ops, c, det)
    w = c.fin.clone().requires_grad_(True)
    bpr, reg = ops.bpr_loss(w, w, c.users, c.pos, c.neg, c.U, REG, True)
    (bpr + reg).backward()
    _same_bits(det, (torch.stack([bpr.detach(), reg.detach()]), w.grad, w.grad), c.tag + " autograd route")


# =================================================================================================== (c) idg_bpr_fused_ex_f32
EX_WIDTHS = [(256, 64), (192, 64), (100, 36), (64, 64), (64, 128), (20, 100)]


@pytest.mark.parametrize("reg_users", [True, False])
@pytest.mark.parametrize("d,de", EX_WIDTHS)
def test_fused_ex_vs_float64(ops, d, de, reg_users):
    """idg_bpr_fused_ex_f32 as idgrec_amd/ngcf.py calls it: bpr_triple_kernel's `else` branch (a.de != a.d, or
    reg_users == 0: the second ego loop, a user row that adds nothing to loss[1]) and bpr_scatter_kernel's `a.de != a.d`
    store of g_final plus its separate loop over the de columns of g_ego; at (64, 64) with reg_users == 0 the one-width
    scatter with `row >= num_users` deciding.  With the item-only regulariser the user rows of g_ego the batch reaches
    are exactly 0.0 in store mode and untouched in accumulate mode."""
    for B, pattern in ((200, "hub"), (64, "edges"), (5, "selfpair")):
        c = _Case("ex", d, B, pattern, de=de, reg_users=reg_users).upload()
        acc = _run(ops, c, ex=True)
        c.check("sorted", *acc[:3])
        _same_bits(acc, _run(ops, c, ex=True), c.tag + " run to run")
        _same_bits(acc, _run(ops, c, ex=True, planned=True), c.tag + " planned")
        _bitmap_claims(ops, c, acc, ex=True)
        if not reg_users:
            ur = c.rows[c.rows < c.U]
            assert len(ur) > 0
            store = _run(ops, c, ex=True, mode="store")
            assert (store[2][ur] == 0).all(), "a reached user row of g_ego is not exactly zero in store mode"
            kept = _run(ops, c, ex=True, prefill_ego_users=1.25)
            assert (kept[2][:c.U] == 1.25).all(), "a user row of g_ego changed in accumulate mode"
            assert torch.equal(kept[2][c.U:], acc[2][c.U:]) and torch.equal(kept[1], acc[1])


def test_fused_ex_refused_calls_write_nothing(ops):
    """deterministic = 0, and g_final == g_ego when the widths differ: a non-zero return, no launch that writes a panel or
    the loss."""
    from idgrec_amd import native

    c = _Case("ex-refuse", 64, 5, "random", de=32).upload()
    ws = ops.bpr_workspace(c.B, c.d, "cuda")
    loss = torch.full((2,), 7.0, device="cuda")
    gf, ge = torch.full((c.n, c.d), 7.0, device="cuda"), torch.full((c.n, c.de), 7.0, device="cuda")

    def call(g_final, g_ego, det):
        return native.lib.idg_bpr_fused_ex_f32(_p(c.fin), c.d, _p(c.ego), c.de, c.U, c.n, _p(c.users), _p(c.pos), _p(c.neg), c.B,
                                               REG, 0, _p(loss), _p(g_final), _p(g_ego), det, None, _p(ws), ops._stream())

    assert call(gf, ge, 0) != 0
    assert call(gf, gf, 1) != 0
    assert call(gf, gf, native.IDG_BPR_PLANNED) != 0
    torch.cuda.synchronize()
    assert (loss == 7.0).all() and (gf == 7.0).all() and (ge == 7.0).all()
    assert call(gf, ge, 1) == 0  # the same arguments with distinct panels are taken


# ============================================================================================================= (d) saturation
@pytest.mark.parametrize("det", [1, 0])
def test_saturated_sigmoid_next_to_the_guard(ops, det):
    """d = 64, B = 200 with distinct users; the user rows of the 50 triples with the largest |x| (the smallest factors, so
    that the rescaled rows do not take over the scale of the item gradients) are rescaled so that x lands near +-17 (float32
    sig rounds to 1 or 1 - 2^-24, 1 - sig to 0 or 2^-24), +-40 and +-100 (expf overflows to inf: sig is exactly 0; or sig is
    exactly 1): -log(sig + 1e-7) and sig (1 - sig) / (sig + 1e-7) must stay finite and inside the band."""
    d, B = 64, 200
    c = _Case("saturate", d, B, "distinct")
    users, pos, neg = c.ids_np
    f = c.fin_np.astype(np.float64)
    x = (f[users] * (f[c.U + pos] - f[c.U + neg])).sum(axis=1)
    quarter = np.argsort(-np.abs(x))[:B // 4]
    targets = np.resize(np.array([17.0, -17.0, 40.0, -40.0, 100.0, -100.0]), B // 4)
    c.fin_np[users[quarter]] = (f[users[quarter]] * (targets / x[quarter])[:, None]).astype(np.float32)
    c.upload()
    f = c.fin_np.astype(np.float64)
    x = (f[users] * (f[c.U + pos] - f[c.U + neg])).sum(axis=1)
    assert np.abs(np.abs(x[quarter]) - np.abs(targets)).max() < 1e-3 and np.abs(np.delete(x, quarter)).max() < 17
    with np.errstate(over="ignore"):
        sig = np.float32(1) / (np.float32(1) + np.exp(-x.astype(np.float32)))  # the kernel's expression, in float32
    assert (sig == 0).any() and (sig == 1).any()
    loss, gf, ge, _ = _run(ops, c, det=det)
    assert torch.isfinite(loss).all() and torch.isfinite(gf).all() and torch.isfinite(ge).all()
    c.check("sorted" if det else "atomic", loss, gf, ge)


# ============================================================================================================= (e) sort routes
def _plan_lists(ws, B):
    """The sorted keys and slots of the workspace (bpr_layout: coef [B] | loss terms [B] | squares [3B] | keys [3B] | slots
    [3B] | SORTED keys [3B] | SORTED slots [3B] | scratch, every region aligned to 256 bytes)."""
    al = lambda x: (x + 255) // 256 * 256  # noqa: E731
    off = al(B * 4) * 2 + al(B * 12) * 3
    raw = ws.cpu().numpy()
    return raw[off: off + 12 * B].view(np.int32), raw[off + al(B * 12): off + al(B * 12) + 12 * B].view(np.int32)


# n = 500: slot_bits + row_bits <= 22, 32-bit keys.  n = 2^22 + 37: row_bits = 23, 64-bit keys once slot_bits >= 9, that is
# from 3B = 1023 on (3B = 3, 63, 66 still pack into 32 bits).  n = 2^31 - 1: row_bits = 31, 64-bit keys at EVERY size — the
# plan needs no panel, so the largest table the entry point takes costs nothing.
PLAN_N = [(300, 200), (1 << 21, (1 << 21) + 37), (1 << 30, (1 << 30) - 1)]


@pytest.mark.parametrize("U,I", PLAN_N)
@pytest.mark.parametrize("B", [1, 21, 22, 341, 342, 683, 1024, 1366, 2730])
def test_sort_plan_routes_equal_the_stable_sort(ops, B, U, I):
    """bpr_sort_plan at 3B <= 8192: launch_lds_sort (3B = 3 below the 64-wide floor, 63, 66, 1023) and launch_rank_sort
    (3B = 1026: a second run of two keys; 2049, 3072, 4098, 8190), each with uint32 and with unsigned long long packed keys
    (`slot_bits + row_bits > 31`).  The sorted keys and slots read back from the workspace are np.lexsort's."""
    n = U + I
    rng = np.random.default_rng(_seed("plan", B, n))
    users, pos, neg = rng.integers(0, U, B), rng.integers(0, I, B), rng.integers(0, I, B)
    neg[0] = I - 1  # row n - 1
    if B > 1:
        users[1], pos[1] = 0, 0  # rows 0 and U
        users[B // 2:] = users[B // 2]  # and one long run of equal keys: the slot bits decide
    slot_bits = max(1, int(np.ceil(np.log2(3 * B))))
    row_bits = max(1, int(np.ceil(np.log2(n))))
    print("  B=%d n=%d: %d-bit packed keys, %s" % (B, n, 64 if slot_bits + row_bits > 31 else 32, "rank sort" if 3 * B > 1024 else "LDS sort"))
    ws = ops.bpr_workspace(B, 4, "cuda")
    ops.bpr_plan_raw(dev(users), dev(pos), dev(neg), U, n, 4, ws=ws)
    torch.cuda.synchronize()
    rows = np.stack([users, U + pos, U + neg], axis=1).reshape(-1)
    order = np.lexsort((np.arange(3 * B), rows))
    got_keys, got_slots = _plan_lists(ws, B)
    assert np.array_equal(got_keys, rows[order].astype(np.int32)), "sorted row keys differ from the stable sort"
    assert np.array_equal(got_slots, order.astype(np.int32)), "sorted slots differ from the stable sort"


@pytest.fixture(scope="module")
def big_panels():
    """U = 2^21 users + I = 2^21 + 37 items at d = 4: two value panels and two gradient panels of 67 MB each, made once and
    freed with the module."""
    U, I, d = 1 << 21, (1 << 21) + 37, 4
    gen = torch.Generator(device="cuda").manual_seed(_seed("big"))
    yield dict(U=U, I=I, d=d, fin=0.3 * torch.randn(U + I, d, device="cuda", generator=gen),
               ego=0.3 * torch.randn(U + I, d, device="cuda", generator=gen),
               gf=torch.empty(U + I, d, device="cuda"), ge=torch.empty(U + I, d, device="cuda"))
    torch.cuda.empty_cache()


@pytest.mark.parametrize("B", [341, 342, 2730])
def test_scatter_consumes_a_64_bit_key_plan(ops, big_panels, B):
    """The scatter on the plans of launch_lds_sort<unsigned long long> (B = 341) and launch_rank_sort<unsigned long long>
    (B = 342, 2730) over 2^22 + 37 rows: stored rows against float64 formed on the device for the rows the batch names
    (the panels compacted to those rows, the ids renumbered); every other row keeps its NaN."""
    p = big_panels
    U, I, d, n = p["U"], p["I"], p["d"], p["U"] + p["I"]
    rng = np.random.default_rng(_seed("big", B))
    users, pos, neg = rng.integers(0, U, B), rng.integers(0, I, B), rng.integers(0, I, B)
    users[0], pos[0], neg[0] = 0, 0, I - 1
    users[1] = U - 1
    hot = rng.choice(B, 70, replace=False)  # a run past 64 slots under 64-bit keys
    pos[hot] = pos[hot[0]]
    users, pos, neg = dev(users), dev(pos), dev(neg)
    gf, ge = p["gf"].fill_(NAN), p["ge"].fill_(NAN)
    touched = torch.zeros((n + 31) // 32, dtype=torch.int32, device="cuda")
    ws = ops.bpr_workspace(B, d, "cuda")
    outs = []
    for det in (1, 2):
        touched.zero_()
        if det == 2:
            ops.bpr_plan_raw(users, pos, neg, U, n, d, ws=ws)
        loss = ops.bpr_fused_raw(p["fin"], p["ego"], users, pos, neg, U, REG, gf, ge, deterministic=det, touched=touched, ws=ws)
        fl = _flags(touched, n)
        rows = torch.nonzero(fl)[:, 0]
        outs.append((loss.clone(), gf[rows], ge[rows], rows))
        gf[rows], ge[rows] = NAN, NAN
        assert torch.isnan(gf).all() and torch.isnan(ge).all(), "a row outside the bitmap was written"
    loss, gfr, ger, rows = outs[0]
    ur, ir = torch.unique(users), torch.unique(torch.cat([pos, neg]))
    assert torch.equal(rows, torch.cat([ur, U + ir])), "the bitmap is not the batch's row set"
    assert rows[0] == 0 and rows[-1] == n - 1
    small = (torch.cat([p["fin"][ur], p["fin"][U + ir]]), torch.cat([p["ego"][ur], p["ego"][U + ir]]), len(ur),
             torch.searchsorted(ur, users), torch.searchsorted(ir, pos), torch.searchsorted(ir, neg), REG)
    l64, gf64, ge64 = ref.bpr64(*small)
    l32, gf32, ge32 = ref.bpr64(*small, dtype=F32)
    tag = "64-bit keys B=%d" % B
    for k in range(2):
        _check("%s loss[%d]" % (tag, k), loss[k], l64[k], l32[k])
    _check(tag + " g_final", gfr, gf64, gf32)
    _check(tag + " g_ego", ger, ge64, ge32)
    _same_bits(outs[0][:3], outs[1][:3], tag + " planned")


def test_merge_sort_route_at_width_100(ops):
    """3B = 8193 > 8192 at d = 100: launch_merge_sort (a second run of ONE key) feeding the scatter's lane tail and second
    pass; B = 2731 also puts more than one term on each of the 1024 virtual threads of the loss reduction — the rider block
    in the scatter launch and idg_bpr_forward_f32's own 1024-thread kernel must give the same bits."""
    c = _Case("merge", 100, 2731, "random").upload()
    det = _run(ops, c)
    c.check("sorted", *det[:3])
    _same_bits(det, _run(ops, c, planned=True), c.tag + " planned")
    _bitmap_claims(ops, c, det)
    one = torch.ones(2, device="cuda")
    gf, ge, loss = torch.zeros_like(c.fin), torch.zeros_like(c.ego), torch.zeros(2, device="cuda")
    ops.bpr_fwd_bwd_raw(c.fin, c.ego, c.users, c.pos, c.neg, c.U, REG, one, gf, ge, loss)
    _same_bits(det, (loss, gf, ge), c.tag + " forward + backward")


# ======================================================================================================== (f) upstream scalars
@pytest.mark.parametrize("planned", [False, True])
@pytest.mark.parametrize("up", [(2.0, -3.0), (0.0, 1.0), (1.0, 1.0)])
@pytest.mark.parametrize("d", [20, 64])
def test_upstream_scalars_vs_float64(ops, d, up, planned):
    """ops.bpr_fwd_bwd_raw (idg_bpr_forward_f32 with its own reduction, then idg_bpr_backward_f32 reading `upstream` on
    the device), sorted in the call and planned; then idg_bpr_backward_f32 with the same scalars AND a touched bitmap.
    (1, 1): bit-identical to idg_bpr_fused_f32, loss included (rider block == stand-alone reduction).  (0, 1): the
    gradient of the final panel has no scale — it is exactly zero."""
    from idgrec_amd import native

    c = _Case("upstream", d, 200, "hub", upstream=up).upload()
    upstream = torch.tensor(up, device="cuda")
    ws = ops.bpr_workspace(c.B, d, "cuda")
    det = 1
    if planned:
        ops.bpr_plan_raw(c.users, c.pos, c.neg, c.U, c.n, d, ws=ws)
        det = 2
    gf, ge, loss = torch.zeros_like(c.fin), torch.zeros_like(c.ego), torch.full((2,), NAN, device="cuda")
    ops.bpr_fwd_bwd_raw(c.fin, c.ego, c.users, c.pos, c.neg, c.U, REG, upstream, gf, ge, loss, deterministic=det, ws=ws)
    (l64, gf64, ge64), (l32, gf32, ge32) = c.refs()
    tag = "%s up=%s%s" % (c.tag, up, " planned" if planned else "")
    for k in range(2):
        _check("%s loss[%d]" % (tag, k), loss[k], l64[k], l32[k])
    if up[0] == 0.0:
        assert (gf64 == 0).all() and (gf == 0).all()
    else:
        _check(tag + " g_final", gf, gf64, gf32)
    _check(tag + " g_ego", ge, ge64, ge32)
    if up == (1.0, 1.0):
        c1 = _Case("upstream", d, 200, "hub").upload()
        _same_bits(_run(ops, c1, planned=planned), (loss, gf, ge), tag + " against the fused call")
    # the same backward storing at a bitmap
    gf2, ge2 = torch.full_like(c.fin, NAN), torch.full_like(c.ego, NAN)
    touched = torch.zeros((c.n + 31) // 32, dtype=torch.int32, device="cuda")
    native.check(native.lib.idg_bpr_backward_f32(_p(c.fin), _p(c.ego), c.U, c.n, _p(c.users), _p(c.pos), _p(c.neg), c.B, d, REG,
                                                 _p(upstream), _p(gf2), _p(ge2), det, _p(touched), _p(ws), ops._stream()),
                 "idg_bpr_backward_f32")
    fl = _flags(touched, c.n)
    assert torch.equal(torch.nonzero(fl)[:, 0], c.rows)
    assert torch.equal(gf2[fl], gf[fl]) and torch.equal(ge2[fl], ge[fl]), tag + ": stored rows differ from accumulated ones"
    assert torch.isnan(gf2[~fl]).all() and torch.isnan(ge2[~fl]).all()


# ===================================================================================================================== (g) Adam
LR = 1e-3


def _adam_inputs(key, shape):
    """A table of embedding size (0.1 * randn: its float32 rounding stays well below an lr-sized step) and three gradients
    randn * 10^uniform(-4, 0)."""
    rng = np.random.default_rng(_seed("adam", key, shape))
    W = dev((0.1 * rng.standard_normal(shape)).astype(np.float32))
    grads = [dev((rng.standard_normal(shape) * 10 ** rng.uniform(-4, 0)).astype(np.float32)) for _ in range(3)]
    return rng, W, grads


def _adam_check(tag, got, want64, want32, W0):
    """got / want: per step (table, exp_avg, exp_avg_sq).  The moments on their own scale; the table through its CHANGE
    over the step, formed in float64 from the stored float32 tables, on the scale max |ref64 change|."""
    prev = (W0, W0.double(), W0)
    for s, (g, w64, w32) in enumerate(zip(got, want64, want32), 1):
        assert all(torch.isfinite(t).all() for t in g)
        _check("%s step %d exp_avg" % (tag, s), g[1], w64[1], w32[1])
        _check("%s step %d exp_avg_sq" % (tag, s), g[2], w64[2], w32[2])
        _check("%s step %d table change" % (tag, s), g[0].double() - prev[0].double(), w64[0] - prev[1],
               w32[0].double() - prev[2].double())
        prev = (g[0], w64[0], w32[0])


@pytest.mark.parametrize("count", [1, 3, 4, 10007, (1 << 21) + 7])
def test_adam_step_vs_float64(ops, count):
    """adam_kernel: the scalar tail alone (1, 3 elements), one float4 (4), one pass of the grid-stride loop with a
    three-element tail (10,007), and n4 > 2048 * 256 — the loop's second pass — with a three-element tail (2^21 + 7)."""
    _, W0, grads = _adam_inputs("step", (count,))
    W, M, V = W0.clone(), torch.zeros_like(W0), torch.zeros_like(W0)
    got = []
    for s, g in enumerate(grads, 1):
        ops.adam_step_raw(W, g, M, V, LR, s)
        got.append((W.clone(), M.clone(), V.clone()))
    _adam_check("adam_step n=%d" % count, got, ref.adam64(W0, grads, lr=LR), ref.adam64(W0, grads, lr=LR, dtype=F32), W0)


def _adam_rows_call(ops, W, G, bitmap, M, V, n, d, step):
    from idgrec_amd import native

    return native.lib.idg_adam_rows_f32(_p(W), _p(G), _p(bitmap), _p(M), _p(V), n, d, LR, 0.9, 0.999, 1e-8, step, ops._stream())


def _bitmap_of(bits):
    n = bits.shape[0]
    words = np.zeros((n + 31) // 32, dtype=np.uint32)
    rows = np.flatnonzero(bits.cpu().numpy())
    np.bitwise_or.at(words, rows >> 5, np.uint32(1) << (rows & 31).astype(np.uint32))
    return dev(words.view(np.int32))


ROWS_SHAPES = [(n, d) for d in (4, 20, 64, 100, 256, 1024) for n in (1, 33, 1000)] + [(40000, 64)]


@pytest.mark.parametrize("n,d", ROWS_SHAPES)
def test_adam_rows_vs_float64(ops, n, d):
    """adam_rows_kernel: d4 = 1 .. 256 (d = 1024, one row per workgroup pass, is the limit); d4 = 5 and 25 do not divide
    256 — the trailing threads of a workgroup return early (`r_in >= rpb`); n = 40,000 at d = 64 is 2500 workgroup passes,
    past the 2048-workgroup cap, so the grid-stride loop runs twice.  About half the rows are flagged, about 5 % of the bits
    flip between steps (a row's moments decay while its gradient is absent), and the gradient buffer holds NaN at every
    unflagged row: it must not be read there."""
    from idgrec_amd import native

    rng, W0, grads = _adam_inputs("rows", (n, d))
    bits = torch.from_numpy(rng.random(n) < 0.5).cuda()
    if n == 1:
        bits[:] = True
    bits_list = []
    for s in range(3):
        if s:
            flip = torch.from_numpy(rng.random(n) < (0.05 if n > 1 else 1.0)).cuda()
            bits = bits ^ flip
        bits_list.append(bits)
    poisoned = [torch.where(b[:, None], g, torch.full_like(g, NAN)) for g, b in zip(grads, bits_list)]
    W, M, V = W0.clone(), torch.zeros_like(W0), torch.zeros_like(W0)
    got = []
    for s, (g, b) in enumerate(zip(poisoned, bits_list), 1):
        native.check(_adam_rows_call(ops, W, g, _bitmap_of(b), M, V, n, d, s), "idg_adam_rows_f32")
        got.append((W.clone(), M.clone(), V.clone()))
    _adam_check("adam_rows n=%d d=%d" % (n, d), got, ref.adam_rows64(W0, poisoned, bits_list, lr=LR),
                ref.adam_rows64(W0, poisoned, bits_list, lr=LR, dtype=F32), W0)


@pytest.mark.parametrize("n,d", [(33, 20), (1000, 64), (1000, 100), (7, 1024), (40000, 64)])
def test_adam_rows_with_all_or_no_bits_is_the_flat_step(ops, n, d):
    """All bits set: idg_adam_rows_f32 == idg_adam_step_f32 on the flattened arrays, bit for bit.  No bit set: ==
    idg_adam_step_f32 on a zero gradient (the NaN-filled gradient buffer is not read)."""
    from idgrec_amd import native

    _, W0, grads = _adam_inputs("rows-flat", (n, d))
    words = (n + 31) // 32
    for name in ("all", "none"):
        a = [W0.clone(), torch.zeros_like(W0), torch.zeros_like(W0)]
        b = [W0.clone(), torch.zeros_like(W0), torch.zeros_like(W0)]
        for s, g in enumerate(grads, 1):
            live = name == "all" or s == 1  # ("none": one real step first, so that there are moments to decay)
            bitmap = torch.full((words,), -1 if live else 0, dtype=torch.int32, device="cuda")
            fed, flat = (g, g) if live else (torch.full_like(g, NAN), torch.zeros_like(g))
            native.check(_adam_rows_call(ops, a[0], fed, bitmap, a[1], a[2], n, d, s), "idg_adam_rows_f32")
            ops.adam_step_raw(b[0].view(-1), flat.view(-1), b[1].view(-1), b[2].view(-1), LR, s)
            for x, y in zip(a, b):
                assert torch.equal(x, y), "%s bits, step %d" % (name, s)
        assert not torch.equal(a[0], W0)


def test_adam_rows_refused_widths_write_nothing(ops):
    """d = 6 (not a multiple of 4) and d = 1028 (d / 4 > 256 threads): a non-zero return before any launch."""
    for d in (6, 1028):
        n = 8
        W, G, M, V = (torch.full((n, d), 7.0, device="cuda") for _ in range(4))
        bitmap = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        assert _adam_rows_call(ops, W, G, bitmap, M, V, n, d, 1) != 0
        torch.cuda.synchronize()
        assert (W == 7.0).all() and (M == 7.0).all() and (V == 7.0).all()
