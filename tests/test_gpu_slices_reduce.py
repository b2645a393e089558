"""The published order of the library's one slice reduction (idg::slices_reduce -> wgrad_reduce_kernel, idg_dense.hip) as the
fused layer backwards reach it: idg_ngcf_layer_bwd_f32, idg_gccf_layer_bwd_f32 and idg_gcmc_layer_bwd_f32.

The workspace layout this file relies on: after the call the entry point has left its row slices at the START of `ws` as
float32 [slices][count], slices = min(ceil(n / 64), 512) (one per persistent workgroup), count = the length of w_grads
(8320 for NGCF, 4160 for LR-GCCF, 8320 for GCMC).  w_grads is their sum in this order and no other:
    lane group g of 16 adds the slices g, g + 16, g + 32, ... ascending (eight at a time, slices past the end as + 0.f),
    then the 16 group sums are added g = 0 .. 15.
The test reads `ws` back, adds the slices on the CPU in float32 in that order and asserts torch.equal with w_grads.

n (slices): 1 (1: a single slice), 1085 (17: one group gets a second slice), 8257 (130: a second pass of the 8 x 16 loop,
partly filled), 32773 (512 from 513 blocks: the cap, and a persistent workgroup that takes two blocks).  p = 0.1 and inputs
drawn N(0, 1): no partial sum is subnormal."""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests.test_gpu_ngcf import SLOPE, STREAMS, _ok, _p, _randn, _rng  # noqa: E402

D = 64
P = 0.1
SIZES = [(1, 1), (1085, 17), (8257, 130), (32773, 512)]
COUNT = {"ngcf": 2 * D * D + 2 * D, "gccf": D * D + D, "gcmc": 2 * (D * D + D)}


@pytest.fixture(scope="module")
def ops():
    import idgrec_amd.ops as ops_

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return ops_


@pytest.fixture(scope="module")
def lib(ops):
    from idgrec_amd import native

    return native.lib


def _sum_in_published_order(part):
    """part: float32 CPU tensor [slices, count]."""
    slices, count = part.shape
    zero = torch.zeros(count, dtype=torch.float32)
    groups = []
    for g in range(16):
        t = zero.clone()
        for s0 in range(g, slices, 8 * 16):
            for q in range(8):
                s = s0 + 16 * q
                t = t + (part[s] if s < slices else zero)
        groups.append(t)
    out = groups[0]
    for g in range(1, 16):
        out = out + groups[g]
    return out


def _backward(model, ops, lib, n, ws):
    """Runs the model's forward and backward on fixed inputs; returns w_grads."""
    rng = _rng("slices", model, n)
    seed, sid = STREAMS[n % 2]
    st = ops._stream()
    nan = lambda *shape: torch.full(shape, float("nan"), device="cuda")  # noqa: E731
    side, gE = _randn(rng, (n, D)), _randn(rng, (n, D))
    W1, W2, b1, b2 = _randn(rng, (D, D)), _randn(rng, (D, D)), _randn(rng, (D,)), _randn(rng, (D,))
    gs, wg = nan(n, D), nan(COUNT[model])
    if model == "ngcf":
        ego, E, N, gg = _randn(rng, (n, D)), nan(n, D), nan(n, D), nan(n, D)
        _ok(lib.idg_ngcf_layer_fwd_f32(_p(side), _p(ego), _p(W1), _p(W2), _p(b1), _p(b2), n, D, SLOPE, P, seed, sid, _p(E), _p(N), D, st),
            "idg_ngcf_layer_fwd_f32")
        _ok(lib.idg_ngcf_layer_bwd_f32(_p(E), _p(gE), None, D, None, _p(side), _p(ego), _p(W1), _p(W2), n, D, SLOPE, P, seed, sid, _p(gs),
                                       _p(gg), _p(wg), _p(ws), st), "idg_ngcf_layer_bwd_f32")
    elif model == "gccf":
        _ok(lib.idg_gccf_layer_bwd_f32(_p(gE), None, D, None, _p(side), _p(W1), n, D, P, seed, sid, _p(gs), _p(wg), _p(ws), st),
            "idg_gccf_layer_bwd_f32")
    else:
        T, N = nan(n, D), nan(n, D)
        _ok(lib.idg_gcmc_layer_fwd_f32(_p(side), _p(W1), _p(b1), _p(W2), _p(b2), n, D, SLOPE, P, seed, sid, _p(T), _p(N), D, st),
            "idg_gcmc_layer_fwd_f32")
        _ok(lib.idg_gcmc_layer_bwd_f32(_p(T), _p(gE), None, D, None, _p(side), _p(W1), _p(b1), _p(W2), n, D, SLOPE, P, seed, sid, _p(gs),
                                       _p(wg), _p(ws), st), "idg_gcmc_layer_bwd_f32")
    return wg


@pytest.mark.parametrize("n,slices", SIZES)
@pytest.mark.parametrize("model", ["ngcf", "gccf", "gcmc"])
def test_w_grads_are_the_slices_added_in_the_published_order(ops, lib, model, n, slices):
    assert slices == min((n + 63) // 64, 512)
    count = COUNT[model]
    ws_floats = int(getattr(lib, "idg_%s_layer_bwd_workspace_bytes" % model)(D)) // 4
    assert ws_floats >= 512 * count
    ws = torch.full((ws_floats,), float("nan"), device="cuda")
    wg = _backward(model, ops, lib, n, ws).cpu()
    part = ws[:slices * count].cpu().view(slices, count)
    assert torch.isfinite(part).all(), "a slice the reduction reads was not written"
    if slices < 512:
        assert torch.isnan(ws[slices * count:]).all(), "the workspace was written past its slices"
    expect = _sum_in_published_order(part)
    print("  %s n=%d: %d slices of %d, max |w_grads| %.3e, elements differing %d" %
          (model, n, slices, count, float(wg.abs().max()), int((wg != expect).sum())))
    assert torch.isfinite(wg).all()
    assert torch.equal(wg, expect)
