"""Shared by tests/test_sem_train_host.py, tests/test_sem_train_gpu.py and tests/golden/make_golden_train_head.py: the semantic
head (proj -> FSQEncoder) restated in plain torch -- differentiable, in any dtype, in the reference's exact order (fsq.py:98-119:
zb + (q - zb).detach(), the index recomputed from zq_low) -- the head's dropout mask in numpy from the contract's text
(include/edtts.h: stream word 0x40000, positions as sites 2 and 3), the training cases and their oracle gradients (fp64: the arbiter,
fp32: the yardstick), each computed once and never modified.

A rounding decision that differs between the fp32 and the fp64 oracle would inflate E_ref and hide a failure, so every case (under
its dropout seeds) is chosen such that every FSQ coordinate of every frame has an fp64 decision margin >= MIN_MARGIN: FEATURE_SEED and
DROP_SEEDS below were searched on the CPU for that, and tests/test_sem_train_host.py asserts it."""
import functools

import numpy as np
import torch

import dropout_util as DU
import train_util as TU
from dropout_util import field, philox4x32_10, scale, seeds_of, threshold
from oracle import edtts_oracle as O
from edge_diffusion_tts_amd.synth import synth_hubert_features, synth_semantic_head
from train_util import MARGIN, rel_err  # noqa: F401  (re-exported)

SEM_STREAM = 0x40000
MIN_MARGIN = 1e-4
KEYS = ("w1", "b1", "lng", "lnb", "w3", "b3", "wd", "bd", "wu", "bu")

# name -> (in_dim (0: FSQEncoder alone), S, levels, dropout p or None (None: the 4-module proj), B, T)
CASES = {
    "H1": (768, 128, [4, 4, 3, 3, 2, 2, 2, 2], None, 2, 37),
    "H2": (256, 64, [7, 5, 3], 0.2, 3, 50),
    "H3": (48, 16, [8, 6, 5, 5, 5], 0.5, 1, 5),
    "H4": (0, 32, [2] * 16, None, 2, 33),
    "H5": (128, 64, [7, 5, 3], None, 4, 175),
}
WEIGHT_SEED = {"H1": 1, "H2": 2, "H3": 3, "H4": 4, "H5": 5}
# searched on the CPU (tests/test_sem_train_host.py::test_margin_condition re-checks them): the first feature seed >= 100 at which the
# margin condition holds without dropout and under each of the case's dropout seeds
FEATURE_SEED = {"H1": 100, "H2": 100, "H3": 100, "H4": 100, "H5": 100}
# dropout: the seeds an encoder whose dropout_generator is torch.Generator().manual_seed(g) draws first, g in DROP_GENS
DROP_GENS = {"H2": (11, 12), "H3": (11, 12)}
DROP_SEEDS = {k: tuple(seeds_of(g)[0] for g in v) for k, v in DROP_GENS.items()}
H2_LENGTHS = (50, 17, 1)


def head_keep(seed, p, rows, width):
    """bool [rows, width]: the keep mask of the head's dropout site (row m = b T + t, column n: c0 = n >> 3, c1 = m, c2 = 0x40000,
    c3 = 0, field n & 7)."""
    m = np.arange(rows, dtype=np.int64).reshape(rows, 1)
    n = np.arange(width, dtype=np.int64).reshape(1, width)
    words = philox4x32_10((seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF), (n >> 3, m, SEM_STREAM, 0))
    return field(words, (n & 7) + 0 * m) >= threshold(p)


def head_multiplier(seed, p, B, T, width, dtype):
    keep = head_keep(seed, p, B * T, width)
    return (torch.from_numpy(np.ascontiguousarray(keep)).to(dtype) * torch.tensor(scale(p), dtype=dtype)).reshape(B, T, width)


def fsq_encoder(p, z, levels):
    """FSQEncoder.forward: (z_q, idx, zb)."""
    lv = torch.tensor(levels, dtype=torch.int32)
    half = ((lv.float() - 1) / 2).to(z.dtype)
    basis = torch.cumprod(torch.tensor([1] + list(levels)[:-1], dtype=torch.int64), dim=0)
    zb = torch.tanh(torch.nn.functional.linear(z, p["wd"], p["bd"]))
    q = torch.round((zb + 1) * half)
    q = torch.minimum(torch.clamp(q, min=0), (lv.float() - 1).to(z.dtype))
    q = q / half - 1
    zq_low = zb + (q - zb).detach()
    idx = (((zq_low + 1) * half).round().long() * basis).sum(-1)
    return torch.nn.functional.linear(zq_low, p["wu"], p["bu"]), idx, zb


def head_forward(p, x, levels, mult=None):
    """proj (Linear, GELU, LayerNorm, [x mult], Linear) -> FSQEncoder; without "w1" in p the quantizer alone (x is z).
    Returns (z_q, idx, zb)."""
    F = torch.nn.functional
    if "w1" in p:
        a = F.layer_norm(F.gelu(F.linear(x, p["w1"], p["b1"])), (p["lng"].shape[0],), p["lng"], p["lnb"], 1e-5)
        if mult is not None:
            a = a * mult
        x = F.linear(a, p["w3"], p["b3"])
    return fsq_encoder(p, x, levels)


def margin_of(zb64, levels):
    """per frame: min over the FSQ coordinates of |frac((zb + 1) half) - 0.5| (fp64)"""
    half = (torch.tensor(levels, dtype=torch.float64) - 1) / 2
    s = (zb64.double() + 1) * half
    return ((s - torch.floor(s)) - 0.5).abs().min(-1).values


def weights_of(proj_sd, q_sd):
    """canonical names -> tensors from synth_semantic_head's two state dicts (either proj layout; proj_sd None: the quantizer alone)"""
    out = {}
    if proj_sd is not None:
        last = "4" if "4.weight" in proj_sd else "3"
        out.update(w1=proj_sd["0.weight"], b1=proj_sd["0.bias"], lng=proj_sd["2.weight"], lnb=proj_sd["2.bias"],
                   w3=proj_sd[last + ".weight"], b3=proj_sd[last + ".bias"])
    out.update(wd=q_sd["proj_down.weight"], bd=q_sd["proj_down.bias"], wu=q_sd["proj_up.weight"], bu=q_sd["proj_up.bias"])
    return out


def param_names(in_dim, dropout_layout, prefix="vq."):
    """canonical name -> the parameter's name in SemanticEncoder (FSQEncoder alone: prefix "")"""
    names = {"wd": prefix + "proj_down.weight", "bd": prefix + "proj_down.bias", "wu": prefix + "proj_up.weight", "bu": prefix + "proj_up.bias"}
    if in_dim:
        last = "4" if dropout_layout else "3"
        names.update(w1="proj.0.weight", b1="proj.0.bias", lng="proj.2.weight", lnb="proj.2.bias", w3=f"proj.{last}.weight", b3=f"proj.{last}.bias")
    return names


@functools.lru_cache(maxsize=None)
def case(name, feature_seed=None):
    """(in_dim, S, levels, p, B, T, proj state dict or None, quantizer state dict, features [B, T, in_dim or S], C [B, T, S])"""
    in_dim, S, levels, p, B, T = CASES[name]
    proj_sd, q_sd = synth_semantic_head(in_dim or 16, S, levels, seed=WEIGHT_SEED[name], dropout_layout=p is not None)
    fs = FEATURE_SEED[name] if feature_seed is None else feature_seed
    x = synth_hubert_features(B, T, in_dim or S, fs)
    if not in_dim:
        proj_sd, x = None, 1.5 * x
    C = torch.randn(B, T, S, generator=torch.Generator().manual_seed(B * 1000 + T))
    return in_dim, S, levels, p, B, T, proj_sd, q_sd, x, C


def run_oracle(w, x, levels, C, dtype, mult=None, lengths=None, want_dx=False):
    """loss (z_q . C).sum() -> (gradients by canonical name [+ "d_z"], z_q, idx, zb).  lengths: the utterances are trimmed to their
    lengths and concatenated (what the ragged call must equal); z_q / idx / zb are then those of the concatenation."""
    p = {k: v.to(dtype).clone().requires_grad_(True) for k, v in w.items()}
    xx = x.to(dtype).clone().requires_grad_(want_dx)
    mm = None if mult is None else mult.to(dtype)
    cc = C.to(dtype)
    if lengths is not None:
        sel = torch.cat([torch.arange(n) + b * x.shape[1] for b, n in enumerate(lengths)])
        flat = lambda t: None if t is None else t.reshape(1, -1, t.shape[-1])[:, sel]  # noqa: E731
        zq, idx, zb = head_forward(p, flat(xx), levels, flat(mm))
        cc = flat(cc)
    else:
        zq, idx, zb = head_forward(p, xx, levels, mm)
    (zq * cc).sum().backward()
    g = {k: v.grad for k, v in p.items()}
    if want_dx:
        g["d_z"] = xx.grad
    return g, zq.detach(), idx, zb.detach()


@functools.lru_cache(maxsize=None)
def oracle_pair(name, drop_seed=None, lengths=None, feature_seed=None):
    """(fp64 gradients, E_ref per tensor, median E_ref, fp32 z_q, fp64 idx, fp32 idx, fp64 margin per frame) of a case; drop_seed:
    the case's p with that seed's mask (None: no dropout, as .eval())."""
    in_dim, S, levels, p, B, T, proj_sd, q_sd, x, C = case(name, feature_seed)
    w = weights_of(proj_sd, q_sd)
    out = {}
    for dtype in (torch.float64, torch.float32):
        mult = None if drop_seed is None else head_multiplier(drop_seed, p, B, T, S, dtype)
        out[dtype] = run_oracle(w, x, levels, C, dtype, mult, lengths, want_dx=not in_dim)
    g64, _, idx64, zb64 = out[torch.float64]
    g32, zq32, idx32, _ = out[torch.float32]
    e_ref = {k: rel_err(g32[k], g64[k]) for k in g64}
    return g64, e_ref, float(torch.tensor(sorted(e_ref.values())).median()), zq32, idx64, idx32, margin_of(zb64, levels)


def check_against_oracle(got, g64, e_ref, med, what):
    """`got`: {canonical name: gradient}.  Every gradient within the bar E <= MARGIN * max(E_ref, median E_ref); returns the worst
    ratio after printing every one."""
    assert set(got) == set(g64), sorted(set(got) ^ set(g64))
    worst, bad = 0.0, []
    for k, v in g64.items():
        assert got[k] is not None, f"{what}: {k} has no gradient"
        assert float(v.abs().max()) > 0, f"{what}: {k} has an all-zero fp64 gradient (a vacuous comparison)"
        assert tuple(got[k].shape) == tuple(v.shape), (k, got[k].shape, v.shape)
        e = rel_err(got[k], v)
        bar = max(e_ref[k], med)
        print(f"{what} {k}: E {e:.2e}  E_ref {e_ref[k]:.2e}  ratio {e / bar:.2f}")
        worst = max(worst, e / bar)
        if not e <= MARGIN * bar:
            bad.append((k, e, e_ref[k]))
    print(f"{what}: worst ratio {worst:.2f} (median E_ref {med:.2e})")
    assert not bad, bad
    return worst


# --------------------------------------------------------------------------------------------------- head into decoder
# The head 64 -> cfg.semantic_dim with the default levels (Dropout layout) feeding the decoder of train_util case G4 through
# sem_features: one loss, one backward.  E2E_FEATURE_SEED: searched like FEATURE_SEED, without dropout and under E2E_GENS.
E2E_IN_DIM, E2E_WEIGHT_SEED, E2E_FEATURE_SEED, E2E_P = 64, 6, 100, 0.2
E2E_GENS = (21, 22)  # dropout_generator seeds of (encoder, decoder)


@functools.lru_cache(maxsize=None)
def e2e_case(feature_seed=None):
    """(cfg, decoder state dict, decoder inputs, head weights by canonical name, features [B, S, 64])"""
    cfg, sd, inp = TU.case("G4")
    B, S = inp["f"].shape[0], inp["f"].shape[1]
    proj_sd, q_sd = synth_semantic_head(E2E_IN_DIM, cfg.semantic_dim, cfg.fsq_levels, seed=E2E_WEIGHT_SEED, dropout_layout=True)
    h = synth_hubert_features(B, S, E2E_IN_DIM, E2E_FEATURE_SEED if feature_seed is None else feature_seed)
    return cfg, sd, inp, proj_sd, q_sd, h


def _e2e_grads(dtype, dropout, feature_seed=None):
    cfg, sd, inp, proj_sd, q_sd, h = e2e_case(feature_seed)
    w = {k: v.to(dtype).clone().requires_grad_(True) for k, v in weights_of(proj_sd, q_sd).items()}
    prm = {k: (v.to(dtype).clone().requires_grad_(k not in TU.BUFFERS) if v.is_floating_point() else v) for k, v in sd.items()}
    x = inp["x"].to(dtype).clone().requires_grad_(True)
    B, S = h.shape[0], h.shape[1]
    mult = None
    if dropout:
        mult = head_multiplier(seeds_of(E2E_GENS[0])[0], E2E_P, B, S, cfg.semantic_dim, dtype)
    zq, idx, zb = head_forward(w, h.to(dtype), cfg.fsq_levels, mult)
    if dropout:
        out = DU.decoder_forward(prm, x, inp["t"], None, inp["si"], zq, heads=cfg.heads, window=cfg.attn_window_size, p=E2E_P,
                                 seed=seeds_of(E2E_GENS[1])[0])
    else:
        out = O.decoder_forward(prm, x, inp["t"], None, inp["si"], zq, heads=cfg.heads, window=cfg.attn_window_size)
    ((out - inp["target"].to(dtype)) ** 2).mean().backward()
    g = {k: v.grad for k, v in prm.items() if v.is_floating_point() and k not in TU.BUFFERS}
    g["d_x"] = x.grad
    g.update({"head." + k: v.grad for k, v in w.items()})
    return g, idx, zb.detach()


@functools.lru_cache(maxsize=None)
def e2e_oracle(dropout, feature_seed=None):
    """(fp64 gradients -- decoder parameters by name, "d_x", "head.<canonical name>" --, E_ref, median E_ref, fp64 idx, fp32 idx, margin)"""
    g64, idx64, zb64 = _e2e_grads(torch.float64, dropout, feature_seed)
    g32, idx32, _ = _e2e_grads(torch.float32, dropout, feature_seed)
    e_ref = {k: rel_err(g32[k], g64[k]) for k in g64 if g64[k] is not None}
    return g64, e_ref, float(torch.tensor(sorted(e_ref.values())).median()), idx64, idx32, margin_of(zb64, e2e_case(feature_seed)[0].fsq_levels)
