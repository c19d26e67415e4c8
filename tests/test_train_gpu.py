"""Training on the GPU: EdgeDiffusionDecoder(kernels="generic", autograd=True) against torch.autograd through the CPU oracle.
The fp64 oracle is the arbiter, the fp32 oracle the yardstick: per gradient tensor E(g) = max|g - g64| / max|g64| must stay within
MARGIN = 4 times max(E_ref(g), median E_ref), E_ref being the fp32 oracle's own error (train_util.check_against_oracle).
Run on the GPU box: python -m pytest tests -m gpu."""
import pytest
import torch

from conftest import max_abs
from edge_diffusion_tts_amd import CFG, DiffusionSchedule, EdgeDiffusionDecoder, native, synth_state_dict
from oracle import edtts_oracle as O
from train_util import BUFFERS, CASES, MARGIN, case, check_against_oracle, oracle_pair, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
FWD_TOL = 1e-4  # tests/test_generic_gpu.py: single forward vs the fp32 oracle


def cu(t):
    return None if t is None else t.to(DEV)


def make(cfg, sd, autograd=True):
    dec = EdgeDiffusionDecoder(cfg, kernels="generic", autograd=autograd)
    dec.load_state_dict(sd)
    return dec.to(DEV).eval()


def leaves(inp):
    x = cu(inp["x"]).requires_grad_(True)
    f = None if inp["f"] is None else cu(inp["f"]).requires_grad_(True)
    return x, f


def loss_of(dec, inp, x, f, which=""):
    eps = dec(x, cu(inp["t" + which]), cu(inp["sem"]), cu(inp["si"]), f)
    return ((eps - cu(inp["target" + which])) ** 2).mean()


def collect(dec, x, f):
    got = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in dec.named_parameters()}
    got["d_x"] = x.grad.detach().clone()
    if f is not None:
        got["d_sem_features"] = f.grad.detach().clone()
    return got


def run(name, two=False, dec=None):
    cfg, sd, inp = case(name)
    dec = dec or make(cfg, sd)
    dec.zero_grad(set_to_none=True)
    x, f = leaves(inp)
    loss = loss_of(dec, inp, x, f)
    if two:
        loss = loss + loss_of(dec, inp, x, f, "2")
    loss.backward()
    return dec, collect(dec, x, f)


@pytest.mark.parametrize("name", list(CASES))
def test_gradients_against_the_fp64_oracle(name):
    """Worst ratio E / max(E_ref, median E_ref) measured on MI355X: see DESIGN.md section 19."""
    g64, _, e_ref, med = oracle_pair(name)
    _, got = run(name)
    check_against_oracle(got, g64, e_ref, med, name)
    cfg = case(name)[0]
    none = {k for k, v in got.items() if v is None}
    want = set()
    if case(name)[2]["f"] is not None:
        want.add("token_emb.weight")
    else:
        want |= {"sem_proj.weight", "sem_proj.bias"}
    if case(name)[2]["si"] is None or not cfg.use_adaln:
        want.add("step_emb.weight")
    if not cfg.use_adaln:
        want |= {"time_emb.1.weight", "time_emb.1.bias", "time_emb.3.weight", "time_emb.3.bias"}
    assert none == want, (sorted(none), sorted(want))


def test_g4_rows_span_three_uneven_dw_slabs():
    _, B, T, _, _, _ = CASES["G4"]
    rows = native.train_dw_slab_rows(B * T)
    assert B * T == 750 and (B * T + rows - 1) // rows >= 3 and (B * T) % rows != 0


@pytest.mark.parametrize("name", list(CASES))
def test_training_forward_is_the_inference_forward(name):
    cfg, sd, inp = case(name)
    train, infer = make(cfg, sd), make(cfg, sd, autograd=False)
    args = (cu(inp["x"]), cu(inp["t"]), cu(inp["sem"]), cu(inp["si"]), cu(inp["f"]))
    a = train(*args)
    assert a.requires_grad and a.grad_fn is not None
    b = infer(*args)
    assert not b.requires_grad
    assert torch.equal(a.detach(), b)
    with torch.no_grad():  # the autograd decoder's own no-grad branch is that call too
        assert torch.equal(train(*args), b)


def test_backward_is_reproducible_and_reads_no_workspace():
    dec, a = run("G4")
    _, b = run("G4", dec=dec)
    # a second forward on the same shape (other inputs: it overwrites the shared workspace) between a forward and its backward
    cfg, sd, inp = case("G4")
    dec.zero_grad(set_to_none=True)
    x, f = leaves(inp)
    loss = loss_of(dec, inp, x, f)
    other = dec(cu(inp["target"]), cu(inp["t2"]), None, cu(inp["si"]), cu(inp["f"]) * 0.5)
    loss.backward()
    c = collect(dec, x, f)
    assert other.grad_fn is not None  # (it ran the training forward, on the same cached workspace)
    for k in a:
        if a[k] is None:
            assert b[k] is None and c[k] is None
        else:
            assert torch.equal(a[k], b[k]), k
            assert torch.equal(a[k], c[k]), k


def test_two_forwards_one_backward():
    g64, _, e_ref, med = oracle_pair("G4", two=True)
    _, got = run("G4", two=True)
    check_against_oracle(got, g64, e_ref, med, "G4 two forwards")


def test_optimiser_step_and_grad_accumulation():
    cfg, sd, inp = case("G4")
    dec = make(cfg, sd)
    # accumulation: two backwards into .grad == the sum of the two single gradients, whichever comes first
    single = []
    for which in ("", "2"):
        dec.zero_grad(set_to_none=True)
        x, f = leaves(inp)
        loss_of(dec, inp, x, f, which).backward()
        single.append(collect(dec, x, f))
    for order in (("", "2"), ("2", "")):
        dec.zero_grad(set_to_none=True)
        x, f = leaves(inp)
        for which in order:
            loss_of(dec, inp, x, f, which).backward()
        acc = collect(dec, x, f)
        first, second = (single[0], single[1]) if order[0] == "" else (single[1], single[0])
        for k, v in acc.items():
            if v is not None:
                assert torch.equal(v, first[k] + second[k]), (order, k)
    # one AdamW step, then the inference call reads the new weights (the _version-based re-pack)
    before = {k: p.detach().clone() for k, p in dec.named_parameters()}
    opt = torch.optim.AdamW(dec.parameters(), lr=1e-2)
    opt.step()
    moved = [k for k, p in dec.named_parameters() if p.grad is not None and not torch.equal(p.detach(), before[k])]
    assert len(moved) > 10
    with torch.no_grad():
        eps = dec(cu(inp["x"]), cu(inp["t"]), cu(inp["sem"]), cu(inp["si"]), cu(inp["f"])).cpu()
    new_sd = {k: v.detach().cpu() for k, v in dec.state_dict().items()}
    ref = O.decoder_forward(new_sd, inp["x"], inp["t"], inp["sem"], inp["si"], inp["f"], heads=cfg.heads, window=cfg.attn_window_size)
    old = O.decoder_forward(sd, inp["x"], inp["t"], inp["sem"], inp["si"], inp["f"], heads=cfg.heads, window=cfg.attn_window_size)
    assert max_abs(eps, ref) < FWD_TOL, max_abs(eps, ref)
    assert max_abs(ref, old) > 100 * FWD_TOL  # the step changed the output: the comparison above saw the new weights


def test_golden_v_prediction_objective(golden):
    """train_v2.train_step's decoder call and loss on the reference's own decoder: the fixture's fp64 arrays are the arbiter, its
    fp32 arrays (the reference itself in fp32) the yardstick."""
    g = golden("train_grads")
    hidden, heads, layers = (int(v) for v in g["cfg"])
    cfg = CFG(device=DEV, hidden=hidden, heads=heads, layers=layers, dropout=0.0)
    dec = EdgeDiffusionDecoder(cfg, kernels="generic", autograd=True)
    dec.load_state_dict(synth_state_dict(cfg, 7))
    dec = dec.to(DEV).train()  # dropout 0: training mode is allowed
    sch = DiffusionSchedule(cfg.diff_steps).to(DEV)
    x0, noise, t, feats = cu(g["x0"]), cu(g["noise"]), cu(g["t"]), cu(g["feats"])
    x_t, _ = sch.q_sample(x0, t, noise)
    v_pred = dec(x_t, t, sem_features=feats, step_idx=torch.zeros(len(t), dtype=torch.long, device=DEV))
    loss = torch.nn.functional.mse_loss(v_pred, sch.get_v_target(x0, noise, t))
    loss.backward()
    names = sorted(k[4:] for k in g if k.startswith("g64."))
    got = {k: p.grad for k, p in dec.named_parameters()}
    assert sorted(k for k, v in got.items() if v is not None) == names
    e_ref = {k: rel_err(g["g32." + k], g["g64." + k]) for k in names}
    e_ref["loss"] = abs(float(g["loss32"]) - float(g["loss64"])) / abs(float(g["loss64"]))
    med = float(torch.tensor(sorted(e_ref.values())).median())
    g64 = {k: g["g64." + k] for k in names}
    g64["loss"] = g["loss64"].reshape(1)
    got = {k: got[k] for k in names}
    got["loss"] = loss.detach().reshape(1)
    check_against_oracle(got, g64, e_ref, med, "golden")
    assert MARGIN == 4.0 and all(b not in names for b in BUFFERS)
