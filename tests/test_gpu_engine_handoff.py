"""The hand-off of an optimizer's Adam state to the fused engines of NGCF, GCCF, BIGCF and EGCF (both encoders), through the
one seam they share (idgrec_amd.modeling.EngineStep._engine_adam): a foreign optimizer is refused and nothing moves; an
optimizer that has already stepped the other way keeps what it accumulated, re-homed into the engine's buffers; disagreeing
step counters are refused.

The `small` golden graph (300 users x 250 items), B = 256 batches of its first sampled epoch, message dropout off, d = 64
and each model's configured layer count: the only shape at which all four engines exist.  The hand-off has no
shape-dependent branch beyond the number of small tensors, which the five cases cover at 0 (EGCF), 2, 6 and 12."""
import os

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 256
#: case -> (plugin, settings on top of configure/<plugin>.txt, number of small tensors)
CASES = {"NGCF": ("NGCF", dict(mess_drop_prob="[0.0, 0.0, 0.0]"), 12), "GCCF": ("GCCF", dict(mess_drop_prob="[0.0, 0.0, 0.0]"), 6),
         "BIGCF": ("BIGCF", {}, 2), "EGCF-parallel": ("EGCF", dict(mode="parallel"), 0),
         "EGCF-alternating": ("EGCF", dict(mode="alternating"), 0)}


def _model(case, tmp_path, g):
    import importlib

    import utility.utility_data.data_loader as data_loader
    import utility.utility_function.tools as tools

    name, extra, n_small = CASES[case]
    cfg = tools.read_configuration(os.path.join(ROOT, "configure", name + ".txt"), name)
    cfg.update({k: str(v) for k, v in extra.items()})
    d = tmp_path / "small"
    d.mkdir(exist_ok=True)
    (d / "train.txt").write_bytes(g["train_txt"].tobytes())
    (d / "test.txt").write_bytes(g["test_txt"].tobytes())
    cfg.update(dataset="small", dataset_path=str(tmp_path) + "/", sparsity_test="0")
    data = data_loader.Data(str(d), cfg)
    tools.set_seed(2024)
    m = getattr(importlib.import_module("models." + name), name)(cfg, data, torch.device("cuda")).to("cuda")
    assert m.fused_step_available() and int(cfg["embedding_size"]) == 64
    params = list(m.parameters())
    assert len(params) == (1 if name == "EGCF" else 2) + n_small
    tri = torch.from_numpy(g["sample1"][:3 * B]).cuda()
    batches = [tuple(tri[i * B:(i + 1) * B, c].contiguous() for c in range(3)) for i in range(3)]
    return m, params, batches, torch.zeros(m.n_fused_losses, device="cuda")


def _moment_buffers(eng):
    """([first-moment buffers], [second-moment buffers]) the engine holds: the panels and, where it has them, the flat ones."""
    return ([t for t in (eng.M, getattr(eng, "SM", None)) if t is not None],
            [t for t in (eng.V, getattr(eng, "SV", None)) if t is not None])


def _inside(t, buffers):
    lo, hi = t.data_ptr(), t.data_ptr() + 4 * t.numel()
    return any(b.data_ptr() <= lo and hi <= b.data_ptr() + 4 * b.numel() for b in buffers)


def _aliases_engine(opt, params, eng):
    first, second = _moment_buffers(eng)
    return all(_inside(opt.state[p]["exp_avg"], first) and _inside(opt.state[p]["exp_avg_sq"], second) for p in params)


@pytest.mark.parametrize("case", list(CASES))
def test_foreign_optimizer_is_refused_and_nothing_moves(case, tmp_path, golden_small):
    m, params, batches, loss = _model(case, tmp_path, golden_small)
    eng = m._fused_engine()
    opt = torch.optim.Adam(params, lr=1e-3)
    held = [t for side in _moment_buffers(eng) for t in side]
    before = [t.detach().clone() for t in params + held]
    assert m.fused_train_step(*batches[0], loss, opt) is False
    assert m._engine_adam(opt) is None
    torch.cuda.synchronize()
    for t, was in zip(params + held, before):
        assert torch.equal(t.detach(), was)
    assert not opt.state  # nor was any state made for it


@pytest.mark.parametrize("case", list(CASES))
def test_state_stepped_the_other_way_is_adopted(case, tmp_path, golden_small):
    """One step by fused_loss_and_grad + optimizer.step() (the moments live in tensors of the optimizer's own), then the seam:
    the `if st:` copy of adopt_adam_state, on the device."""
    from idgrec_amd import ops

    m, params, batches, loss = _model(case, tmp_path, golden_small)
    opt = ops.Adam(params, lr=1e-3)
    m.fused_loss_and_grad(*batches[0])
    opt.step()
    want = [(opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for p in params]
    assert all(int(opt.state[p]["step"]) == 1 for p in params)
    adam = m._engine_adam(opt)
    assert adam is not None and adam[0] is opt.param_groups[0] and adam[1] == 1
    eng = m._fused_engine()
    for p, (wm, wv) in zip(params, want):
        st = opt.state[p]
        assert torch.equal(st["exp_avg"], wm) and torch.equal(st["exp_avg_sq"], wv)
        assert float(wm.abs().max()) > 0
    assert _aliases_engine(opt, params, eng)
    for b in batches[1:]:
        assert m.fused_train_step(*b, loss, opt) is True
        assert torch.isfinite(loss).all()
    assert m._fused_engine() is eng
    assert all(int(opt.state[p]["step"]) == 3 for p in params)
    assert all(torch.isfinite(p.detach()).all() for p in params)
    assert _aliases_engine(opt, params, eng)


@pytest.mark.parametrize("case", list(CASES))
def test_disagreeing_step_counters_are_refused(case, tmp_path, golden_small):
    """One parameter's counter runs one ahead: no step, no parameter moves.  EGCF has ONE parameter: a lone counter has
    nothing to disagree with, and by the hand-off's definition (the common step count) the step is taken from it."""
    from idgrec_amd import ops

    m, params, batches, loss = _model(case, tmp_path, golden_small)
    opt = ops.Adam(params, lr=1e-3)
    assert m.fused_train_step(*batches[0], loss, opt) is True
    opt.state[params[-1]]["step"] += 1
    before = [p.detach().clone() for p in params]
    took = m.fused_train_step(*batches[1], loss, opt)
    torch.cuda.synchronize()
    if len(params) == 1:
        assert took is True and int(opt.state[params[0]]["step"]) == 3
        return
    assert took is False and m._engine_adam(opt) is None
    for p, was in zip(params, before):
        assert torch.equal(p.detach(), was)
    assert [int(opt.state[p]["step"]) for p in params] == [1] * (len(params) - 1) + [2]
