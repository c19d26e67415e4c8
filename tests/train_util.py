"""Shared by tests/test_train_host.py and tests/test_train_gpu.py: the training cases, and gradients of the CPU oracle under
torch.autograd (fp64: the arbiter, fp32: the yardstick).  Each oracle run is computed once per case and never modified."""
import functools

import torch

from edge_diffusion_tts_amd import CFG, synth_state_dict
from oracle import edtts_oracle as O

BUFFERS = ("pos_emb.pe", "context_pos_emb.pe")
MARGIN = 4.0  # tests/test_train_gpu.py: E(g) <= MARGIN * max(E_ref(g), median E_ref)

# name -> (cfg kwargs, B, T, S, context from features?, step_idx given?)
CASES = {
    "G1": (dict(hidden=96, heads=4, attn_window_size=5, ffn_mult=3, use_adaln=False, codebook_size=16, layers=2), 3, 50, 25, False, True),
    "G2": (dict(hidden=50, heads=5, n_mels=45, semantic_dim=7, attn_window_size=3, layers=2), 2, 19, 9, True, True),
    "G3": (dict(hidden=100, heads=4, n_mels=100, semantic_dim=24, attn_window_size=None, layers=2), 2, 33, 17, True, False),
    "G4": (dict(hidden=160, heads=4, attn_window_size=64, layers=2), 5, 150, 75, True, True),
    "G5": (dict(hidden=256, heads=2, layers=1), 2, 64, 31, False, True),
}


@functools.lru_cache(maxsize=None)
def case(name, device="cpu"):
    """(cfg, state dict, inputs) of a case: fixed inputs from a seeded CPU generator."""
    kw, B, T, S, feats, with_step = CASES[name]
    cfg = CFG(device=device, **kw)
    sd = synth_state_dict(cfg, 0)
    g = torch.Generator().manual_seed(B * 1000 + T)
    inp = dict(
        x=torch.randn(B, T, cfg.n_mels, generator=g),
        t=torch.randint(0, 1000, (B,), generator=g),
        t2=torch.randint(0, 1000, (B,), generator=g),
        si=torch.randint(0, 16, (B,), generator=g) if with_step else None,
        sem=None if feats else torch.randint(0, cfg.codebook_size, (B, S), generator=g),
        f=torch.randn(B, S, cfg.semantic_dim, generator=g) if feats else None,
        target=torch.randn(B, T, cfg.n_mels, generator=g),
        target2=torch.randn(B, T, cfg.n_mels, generator=g),
    )
    return cfg, sd, inp


def oracle_grads(cfg, sd, inp, dtype, two=False, loss_fn=None):
    """(loss, {name: gradient or None}) of the oracle under torch.autograd in `dtype`; "d_x" / "d_sem_features" are the input
    gradients.  Loss: ((dec(x, t, ...) - target)^2).mean(), with two=True plus the same on (t2, target2): two forwards, one backward."""
    p = {k: (v.to(dtype).clone().requires_grad_(k not in BUFFERS) if v.is_floating_point() else v) for k, v in sd.items()}
    x = inp["x"].to(dtype).clone().requires_grad_(True)
    f = None if inp["f"] is None else inp["f"].to(dtype).clone().requires_grad_(True)

    def fwd(t):
        return O.decoder_forward(p, x, t, inp["sem"], inp["si"], f, heads=cfg.heads, window=cfg.attn_window_size)

    if loss_fn is not None:
        loss = loss_fn(fwd, x)
    else:
        loss = ((fwd(inp["t"]) - inp["target"].to(dtype)) ** 2).mean()
        if two:
            loss = loss + ((fwd(inp["t2"]) - inp["target2"].to(dtype)) ** 2).mean()
    loss.backward()
    grads = {k: v.grad for k, v in p.items() if v.is_floating_point() and k not in BUFFERS}
    grads["d_x"] = x.grad
    if f is not None:
        grads["d_sem_features"] = f.grad
    return loss.detach(), grads


@functools.lru_cache(maxsize=None)
def oracle_pair(name, two=False):
    """(fp64 gradients, fp32 gradients, E_ref per tensor, median E_ref) of a case, computed once."""
    cfg, sd, inp = case(name)
    _, g64 = oracle_grads(cfg, sd, inp, torch.float64, two)
    _, g32 = oracle_grads(cfg, sd, inp, torch.float32, two)
    e_ref = {k: rel_err(g32[k], g64[k]) for k in g64 if g64[k] is not None}
    return g64, g32, e_ref, float(torch.tensor(sorted(e_ref.values())).median())


def rel_err(g, g64):
    """E(g) = max|g - g64| / max|g64|."""
    return float((g.detach().cpu().double() - g64.double()).abs().max() / g64.double().abs().max())


def check_against_oracle(got, g64, e_ref, med, what):
    """`got`: {name: gradient or None}.  None exactly where the oracle has None; everything else within the bar.  Returns the worst
    ratio E / max(E_ref, median E_ref) after printing every one."""
    assert set(got) == set(g64), (sorted(set(got) ^ set(g64)))
    none_got = sorted(k for k, v in got.items() if v is None)
    none_ref = sorted(k for k, v in g64.items() if v is None)
    assert none_got == none_ref, (none_got, none_ref)
    worst, bad = 0.0, []
    for k, v in g64.items():
        if v is None:
            continue
        assert float(v.abs().max()) > 0, f"{what}: {k} has an all-zero fp64 gradient (a vacuous comparison)"
        assert got[k].shape == v.shape, (k, got[k].shape, v.shape)
        e = rel_err(got[k], v)
        bar = max(e_ref[k], med)
        print(f"{what} {k}: E {e:.2e}  E_ref {e_ref[k]:.2e}  ratio {e / bar:.2f}")
        worst = max(worst, e / bar)
        if not e <= MARGIN * bar:
            bad.append((k, e, e_ref[k]))
    print(f"{what}: worst ratio {worst:.2f} (median E_ref {med:.2e})")
    assert not bad, bad
    return worst
