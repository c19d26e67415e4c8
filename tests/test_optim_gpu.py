"""FusedAdamW on the GPU: parity with clip_grad_norm_ + torch.optim.AdamW (fp64 on the CPU the arbiter, the same torch code in fp32
the yardstick: E <= MARGIN * max(E_ref, median E_ref), train_util.check_against_oracle), reproducibility, skipped parameters and
steps, the EMA teacher and the mirror into the decoder's packed blob.  Run on the GPU box: python -m pytest tests -m gpu."""
import functools

import pytest
import torch

from edge_diffusion_tts_amd import EdgeDiffusionDecoder, FusedAdamW, native, optim
from train_util import BUFFERS, case, check_against_oracle, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
LRS = (3e-3, 1e-2, 5e-4)
SCALES = (1.0, 0.5, 1e-4)  # gradient norms of about 200, 100 and 0.02 against max_norm = 1: clipped, clipped, not clipped
MAX_NORM = 1.0
HYPER = dict(betas=(0.9, 0.98), eps=1e-8)
N_VIEW = 1  # index of the group-0 tensor that is a base[1:] view on the device


def bits(t):
    return t.detach().contiguous().view(torch.int32).clone()


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def problem():
    """Fixed CPU data: parameter values and three gradients per tensor.  Sizes around the 4-wide vector, the wave, the chunk; a matrix;
    tensor 1 becomes a misaligned view on the device (the scalar path, over more than one chunk)."""
    chunk = optim.CHUNK
    shapes = [(1,), (chunk + 7,), (3,), (5,), (63,), (64,), (65,), (chunk - 1,), (chunk + 1,), (2 * chunk + 3,), (33, 17)]
    g = torch.Generator().manual_seed(11)
    params = [torch.randn(s, generator=g) for s in shapes]
    grads = [[torch.randn(s, generator=g) * SCALES[k] for s in shapes] for k in range(3)]
    return params, grads


def groups_of(ps):
    return [dict(params=ps[0::2], weight_decay=0.05), dict(params=ps[1::2], weight_decay=0.0)]


@functools.lru_cache(maxsize=None)
def torch_run(dtype, ema_decay=None, steps=3):
    """clip_grad_norm_(foreach=False) + AdamW(foreach=False) on the CPU in `dtype`: (updates, exp_avg, exp_avg_sq, norms, teachers)."""
    params, grads = problem()
    ps = [p.to(dtype).clone().requires_grad_(True) for p in params]
    teach = [p.to(dtype).clone() * 0.5 for p in params]
    opt = torch.optim.AdamW(groups_of(ps), lr=1.0, foreach=False, **HYPER)
    norms = []
    for k in range(steps):
        for g in opt.param_groups:
            g["lr"] = LRS[k]
        for p, g in zip(ps, grads[k]):
            p.grad = g.to(dtype).clone()
        norms.append(torch.nn.utils.clip_grad_norm_(ps, MAX_NORM, foreach=False).detach().clone())
        opt.step()
        if ema_decay is not None:
            with torch.no_grad():
                for t, p in zip(teach, ps):
                    t.lerp_(p, 1.0 - ema_decay)
    upd = [p.detach() - q.to(dtype) for p, q in zip(ps, params)]
    return upd, [opt.state[p]["exp_avg"] for p in ps], [opt.state[p]["exp_avg_sq"] for p in ps], norms, teach


class Holder(torch.nn.Module):
    def __init__(self, tensors):
        super().__init__()
        self.ps = torch.nn.ParameterList([t if isinstance(t, torch.nn.Parameter) else torch.nn.Parameter(t) for t in tensors])


def device_params():
    params, _ = problem()
    out = []
    for i, p in enumerate(params):
        if i == N_VIEW:
            base = torch.zeros(p.numel() + 1, device=DEV)
            base[1:].copy_(p)
            q = torch.nn.Parameter(base[1:])
            assert q.data_ptr() % 16 == 4
        else:
            q = torch.nn.Parameter(p.to(DEV))
        out.append(q)
    return out


def ours_run(steps=3, sync=True, skip=(), **kw):
    """The same three steps on the GPU.  `skip`: indices of tensors that never get a gradient.  Returns (opt, params, norms)."""
    _, grads = problem()
    ps = device_params()
    opt = FusedAdamW(groups_of(ps), lr=1.0, max_norm=MAX_NORM, **HYPER, **kw)
    dev_grads = [[g.to(DEV) for g in gs] for gs in grads]
    torch.cuda.synchronize()
    norms = []
    for k in range(steps):
        for g in opt.param_groups:
            g["lr"] = LRS[k]
        for i, (p, g) in enumerate(zip(ps, dev_grads[k])):
            p.grad = None if i in skip else g
        norms.append(opt.step())
        if sync:
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    return opt, ps, norms


def bar(got, r64, r32, what):
    e_ref = {k: rel_err(r32[k], r64[k]) for k in r64}
    med = float(torch.tensor(sorted(e_ref.values())).median())
    return check_against_oracle(got, r64, e_ref, med, what)


def named(prefix, tensors):
    return {f"{prefix}.{i}": t for i, t in enumerate(tensors)}


def test_parity_with_torch_clip_and_adamw():
    """Worst ratio E / max(E_ref, median E_ref) measured on MI355X: see DESIGN.md section 24."""
    params, _ = problem()
    u64, m64, v64, n64, _ = torch_run(torch.float64)
    u32, m32, v32, n32, _ = torch_run(torch.float32)
    assert float(n64[0]) > MAX_NORM and float(n64[1]) > MAX_NORM and float(n64[2]) < MAX_NORM  # clipped, clipped, not clipped
    opt, ps, norms = ours_run()
    assert all(n.dim() == 0 and n.is_cuda for n in norms)
    assert opt._read_step() == 3 and opt.skipped_steps() == 0
    upd = [p.detach().cpu() - q for p, q in zip(ps, params)]
    worst = 0.0
    worst = max(worst, bar(named("update", upd), named("update", u64), named("update", u32), "update"))
    worst = max(worst, bar(named("exp_avg", [opt.state[p]["exp_avg"] for p in ps]), named("exp_avg", m64), named("exp_avg", m32), "exp_avg"))
    worst = max(worst, bar(named("exp_avg_sq", [opt.state[p]["exp_avg_sq"] for p in ps]), named("exp_avg_sq", v64), named("exp_avg_sq", v32),
                           "exp_avg_sq"))
    worst = max(worst, bar(named("total_norm", norms), named("total_norm", n64), named("total_norm", n32), "total_norm"))
    print(f"FusedAdamW parity: worst ratio {worst:.2f}")
    # the gradients are read, not rescaled; versions moved once per step
    _, grads = problem()
    assert all(same_bits(p.grad.cpu(), g) for p, g in zip(ps, grads[2]))
    assert all(p._version >= 3 for p in ps)
    # state_dict is AdamW's
    sd = opt.state_dict()
    assert all(set(s) == {"step", "exp_avg", "exp_avg_sq"} and float(s["step"]) == 3.0 for s in sd["state"].values())


def test_steps_are_reproducible_and_need_no_synchronisation():
    a_opt, a, a_n = ours_run(sync=True)
    b_opt, b, b_n = ours_run(sync=True)
    c_opt, c, c_n = ours_run(sync=False)  # three steps enqueued back to back: the pointer tables travel through the pinned ring
    for other_opt, other, other_n in ((b_opt, b, b_n), (c_opt, c, c_n)):
        for p, q in zip(a, other):
            assert same_bits(p, q)
            assert same_bits(a_opt.state[p]["exp_avg"], other_opt.state[q]["exp_avg"])
            assert same_bits(a_opt.state[p]["exp_avg_sq"], other_opt.state[q]["exp_avg_sq"])
        assert all(same_bits(x, y) for x, y in zip(a_n, other_n))


def test_parameters_without_gradient_or_elements_are_untouched():
    params, grads = problem()
    skip = (0, 4, 9)
    opt, ps, _ = ours_run(steps=2, skip=skip)
    for i, p in enumerate(ps):
        if i in skip:
            assert same_bits(p.cpu(), params[i]) and p._version == 0 and p not in opt.state
        else:
            assert not torch.equal(p.cpu(), params[i]) and set(opt.state[p]) == {"exp_avg", "exp_avg_sq"}
    # the stepped ones went exactly where they go when the skipped tensors are not there at all (the clip norm is over them alone)
    keep = [i for i in range(len(params)) if i not in skip]
    empty = torch.zeros(0, device=DEV, requires_grad=True)
    empty.grad = torch.zeros(0, device=DEV)
    qs = device_params()
    sub = [qs[i] for i in keep]
    opt2 = FusedAdamW([dict(params=[q for i, q in zip(keep, sub) if i % 2 == 0] + [empty], weight_decay=0.05),
                       dict(params=[q for i, q in zip(keep, sub) if i % 2 == 1], weight_decay=0.0)], lr=1.0, max_norm=MAX_NORM, **HYPER)
    for k in range(2):
        for g in opt2.param_groups:
            g["lr"] = LRS[k]
        for i, q in zip(keep, sub):
            q.grad = grads[k][i].to(DEV)
        opt2.step()
    torch.cuda.synchronize()
    for i, q in zip(keep, sub):
        assert same_bits(q, ps[i])
    assert empty not in opt2.state and empty._version == 0


def test_zero_grads_zero_fills_the_gradients_it_used():
    _, a, _ = ours_run(steps=2)
    _, b, _ = ours_run(steps=2, zero_grads=True)
    for p, q in zip(a, b):
        assert same_bits(p, q)
        assert float(p.grad.abs().max()) > 0 and q.grad is not None and not bool(q.grad.any())


def test_nan_propagates_without_skip_nonfinite():
    params, grads = problem()
    ps = device_params()
    opt = FusedAdamW(groups_of(ps), lr=1e-3, max_norm=MAX_NORM, **HYPER)
    for i, p in enumerate(ps):
        p.grad = grads[0][i].to(DEV)
    ps[5].grad[7] = float("nan")
    norm = opt.step()
    torch.cuda.synchronize()
    # torch: total_norm NaN -> clip_coef NaN -> every gradient NaN -> every parameter NaN
    assert bool(torch.isnan(norm)) and all(bool(torch.isnan(p).all()) for p in ps)
    assert opt._read_step() == 1 and opt.skipped_steps() == 0


def decoder_setup(name, with_teacher=False, **kw):
    cfg, sd, inp = case(name)
    dec = EdgeDiffusionDecoder(cfg, kernels="generic", autograd=True)
    dec.load_state_dict(sd)
    dec = dec.to(DEV).eval()
    opt = FusedAdamW(dec.parameters(), lr=2e-3, weight_decay=0.01, max_norm=0.5, **kw)
    assert opt.attach_decoder(dec) is True
    teacher = None
    if with_teacher:
        teacher = EdgeDiffusionDecoder(cfg, kernels="generic")
        teacher.load_state_dict({k: (v if k in BUFFERS else v * 0.9) for k, v in sd.items()})
        teacher = teacher.to(DEV).eval()
        opt.attach_ema(dec, teacher, decay=0.9)
    return cfg, inp, dec, opt, teacher


def cu(t):
    return None if t is None else t.to(DEV)


def fwd(dec, inp, which=""):
    return dec(cu(inp["x"]), cu(inp["t" + which]), cu(inp["sem"]), cu(inp["si"]), cu(inp["f"]))


def backward(dec, inp):
    dec.zero_grad(set_to_none=True)
    ((fwd(dec, inp) - cu(inp["target"])) ** 2).mean().backward()


def fresh_blob(dec):
    names, tensors = dec._slot_tensors()
    out = torch.full((native.packed_bytes(dec.dims()),), 0xA5, dtype=torch.uint8, device=DEV)
    native.pack_weights(dec.dims(), [t.contiguous() for t in tensors], out)
    return out


def count_packs(monkeypatch):
    calls = []
    real = native.pack_weights
    monkeypatch.setattr(native, "pack_weights", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


def reloaded_eps(dec, cfg, inp):
    twin = EdgeDiffusionDecoder(cfg, kernels="generic")
    twin.load_state_dict(dec.state_dict())
    twin = twin.to(DEV).eval()
    with torch.no_grad():
        return fwd(twin, inp, "2")


@pytest.mark.parametrize("name", ["G1", "G2"])
def test_step_mirrors_into_the_packed_blob(name, monkeypatch):
    cfg, inp, dec, opt, teacher = decoder_setup(name, with_teacher=True)
    with torch.no_grad():
        fwd(teacher, inp)  # the teacher's blob is packed and current
    backward(dec, inp)
    before = {k: p.detach().clone() for k, p in dec.named_parameters()}
    t_before = {k: p.detach().clone() for k, p in teacher.named_parameters()}
    stepped = {k for k, p in dec.named_parameters() if p.grad is not None}
    assert stepped and stepped != set(before)  # (some parameters do not enter this forward: they must stay as they are)
    opt.step()
    torch.cuda.synchronize()
    assert all(same_bits(p, before[k]) for k, p in dec.named_parameters() if k not in stepped)
    assert not any(same_bits(p, before[k]) for k, p in dec.named_parameters() if k in stepped and float(before[k].abs().max()) > 0)
    # byte for byte what a pack of the updated parameters gives: the zero padding and the buffer tables included
    assert torch.equal(dec._packed, fresh_blob(dec))
    assert torch.equal(teacher._packed, fresh_blob(teacher))
    # the teacher: lerp_ toward the new student where the student was stepped, untouched elsewhere
    t64, t32, got = {}, {}, {}
    for k, p in teacher.named_parameters():
        if k in stepped:
            s = dict(dec.named_parameters())[k].detach().cpu()
            t64[k] = t_before[k].cpu().double().lerp_(s.double(), 1.0 - 0.9) - t_before[k].cpu().double()
            t32[k] = t_before[k].cpu().clone().lerp_(s, 1.0 - 0.9) - t_before[k].cpu()
            got[k] = p.detach().cpu() - t_before[k].cpu()
        else:
            assert same_bits(p, t_before[k]), k
    bar(got, t64, t32, f"{name} teacher")
    calls = count_packs(monkeypatch)
    with torch.no_grad():
        eps = fwd(dec, inp, "2")
        eps_t = fwd(teacher, inp, "2")
    assert calls == [], "the forward after a mirrored step packs nothing"
    assert same_bits(eps, reloaded_eps(dec, cfg, inp))
    assert same_bits(eps_t, reloaded_eps(teacher, cfg, inp))
    # update_ema: every pair, mirrored as well
    opt.update_ema()
    torch.cuda.synchronize()
    assert torch.equal(teacher._packed, fresh_blob(teacher))
    for k, p in teacher.named_parameters():
        if k not in stepped and not torch.equal(before[k], t_before[k]):
            assert not same_bits(p, t_before[k]), k


@pytest.mark.parametrize("name", ["G1", "G2"])
def test_stale_blob_is_not_mirrored(name, monkeypatch):
    cfg, inp, dec, opt, _ = decoder_setup(name)
    backward(dec, inp)
    with torch.no_grad():
        dec.out_proj.bias.add_(0.25)  # by hand, between backward and step: the blob no longer holds the parameters
    stale = dec._packed.clone()
    opt.step()
    torch.cuda.synchronize()
    assert torch.equal(dec._packed, stale), "a stale blob is left alone"
    calls = count_packs(monkeypatch)
    with torch.no_grad():
        eps = fwd(dec, inp, "2")
    assert calls == [1], "the next forward re-packs"
    assert same_bits(eps, reloaded_eps(dec, cfg, inp))
    # from here on the blob is current again and the next step mirrors
    del calls[:]  # (the reloaded twin packed its own blob)
    backward(dec, inp)
    opt.step()
    with torch.no_grad():
        fwd(dec, inp, "2")
    assert calls == []
    assert torch.equal(dec._packed, fresh_blob(dec))


def test_skip_nonfinite_changes_nothing_and_is_counted():
    def run(bad_step):
        cfg, inp, dec, opt, teacher = decoder_setup("G2", with_teacher=True, skip_nonfinite=True)
        with torch.no_grad():
            fwd(teacher, inp)
        backward(dec, inp)
        opt.step()
        if bad_step:
            backward(dec, inp)
            snap = lambda: ([p.detach().clone() for p in dec.parameters()] + [p.detach().clone() for p in teacher.parameters()] +
                            [opt.state[p][k].clone() for p in dec.parameters() if p in opt.state for k in ("exp_avg", "exp_avg_sq")] +
                            [dec._packed.clone(), teacher._packed.clone()])
            before = snap()
            dec.out_proj.weight.grad[3, 5] = float("nan")
            norm = opt.step()
            torch.cuda.synchronize()
            assert bool(torch.isnan(norm))
            assert all(same_bits(a, b) for a, b in zip(before, snap()))
            assert opt._read_step() == 1 and opt.skipped_steps() == 1
        backward(dec, inp)
        opt.step()
        torch.cuda.synchronize()
        assert opt._read_step() == 2
        assert torch.equal(dec._packed, fresh_blob(dec))
        return [p.detach().clone() for p in dec.parameters()] + [p.detach().clone() for p in teacher.parameters()]

    with_bad, without = run(True), run(False)
    assert all(same_bits(a, b) for a, b in zip(with_bad, without))


def test_ema_meets_the_bar_after_two_steps():
    params, grads = problem()
    decay = 0.95
    _, _, _, _, t64 = torch_run(torch.float64, ema_decay=decay, steps=2)
    _, _, _, _, t32 = torch_run(torch.float32, ema_decay=decay, steps=2)
    ps = device_params()
    student = Holder(ps)
    teacher = Holder([p.to(DEV) * 0.5 for p in params])
    opt = FusedAdamW(groups_of(ps), lr=1.0, max_norm=MAX_NORM, **HYPER)
    opt.attach_ema(student, teacher, decay=decay)
    start = [t.detach().clone() for t in teacher.ps]
    for k in range(2):
        for g in opt.param_groups:
            g["lr"] = LRS[k]
        for p, g in zip(ps, grads[k]):
            p.grad = g.to(DEV)
        opt.step()
    torch.cuda.synchronize()
    ref_start = [p * 0.5 for p in params]
    got = named("teacher", [t.detach().cpu() - s for t, s in zip(teacher.ps, ref_start)])
    bar(got, named("teacher", [t - s.double() for t, s in zip(t64, ref_start)]), named("teacher", [t - s for t, s in zip(t32, ref_start)]), "EMA")
    assert all(t._version >= 2 for t in teacher.ps)
    # second run: tensors that are not stepped leave their teachers alone
    skip = (2, 10)
    ps2 = device_params()
    student2, teacher2 = Holder(ps2), Holder([t.clone() for t in start])
    opt2 = FusedAdamW(groups_of(ps2), lr=1e-3, max_norm=MAX_NORM, **HYPER)
    opt2.attach_ema(student2, teacher2, decay=decay)
    for i, (p, g) in enumerate(zip(ps2, grads[0])):
        p.grad = None if i in skip else g.to(DEV)
    opt2.step()
    torch.cuda.synchronize()
    for i, (t, s) in enumerate(zip(teacher2.ps, start)):
        assert same_bits(t, s) == (i in skip), i
