"""Shared by tests/test_objective_host.py and tests/test_objective_gpu.py: the cases of the training objective and its oracle.

The oracle is the reference's own expressions in torch on the CPU -- normalize_mel (utils/audio.py:10-14), q_sample, get_v_target,
predict_x0_from_v / _eps (schedule.py), F.mse_loss and F.cosine_similarity as train_v2.py:135-154 calls them, and the two losses of
training/consistency.py:60-122 -- in two forms.  ``padded`` is the batch expression as the reference writes it.  ``ragged`` trims every
row to its length, evaluates it ALONE (its own statistics, its own cosine) and combines the squared-error sums over the live
elements: it never sees a padded frame, so it says what "padding contributes nothing" means without a mask of its own.  Both run
under torch.autograd in fp64 (the arbiter) and fp32 (the yardstick); each run is computed once per case and never modified."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from edge_diffusion_tts_amd import DiffusionSchedule

T_DIFF = 1000
MARGIN = 4.0  # the project's bar (tests/train_util.py): E <= MARGIN * max(E_ref, median E_ref)
KINDS = ("v", "eps", "distill", "consistency")

# name -> (B, T, M, lengths, T_pred, T_pred2, t, t2)
#   O1        T M = 666 is not a multiple of 4: the per-element path; a row of 2 frames, the shortest with a finite std
#   O2        10400 elements per row: two whole loss chunks of 4096 and a tail; the float4 path
#   O3        the float4 path with a live count (3 x 18 = 54) that is no multiple of 4: a quad straddles the row's end
#   O1-short  the prediction is 3 frames shorter than the mel (the reference's "align sequence lengths")
#   O2-long   ... and 2 frames longer: the unit gradient has frames the mel does not have
CASES = {
    "O1": (3, 37, 18, (37, 20, 2), 37, 37, (1, 999, 500), (700, 1, 999)),
    "O2": (2, 130, 80, (130, 77), 130, 130, (999, 1), (1, 640)),
    "O3": (2, 10, 18, (10, 3), 10, 10, (250, 999), (999, 1)),
    "O1-short": (3, 37, 18, (37, 20, 2), 34, 37, (1, 999, 500), (700, 1, 999)),
    "O2-long": (2, 130, 80, (130, 77), 132, 130, (999, 1), (1, 640)),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """Fixed inputs of a case from a seeded CPU generator; the padding holds ordinary finite values (the GPU tests overwrite it)."""
    B, T, M, lengths, Tp, Tp2, t, t2 = CASES[name]
    g = torch.Generator().manual_seed(B * 1000 + T)
    return dict(
        mel=torch.randn(B, T, M, generator=g) * 1.5 - 4.0,  # a raw log-mel: off-centre, so the normalisation matters
        noise=torch.randn(B, T, M, generator=g),
        pred=torch.randn(B, Tp, M, generator=g),
        pred2=torch.randn(B, Tp2, M, generator=g),
        t=torch.tensor(t), t2=torch.tensor(t2), lengths=torch.tensor(lengths),
    )


@functools.lru_cache(maxsize=None)
def tables(dtype):
    s = DiffusionSchedule(T_DIFF)  # CPU tables, bit-equal to the reference's (tests/test_host_cpu.py)
    return {n: getattr(s, n).to(dtype) for n in ("sqrt_alpha_bar", "sqrt_one_minus_alpha_bar", "sqrt_recip_alpha_bar", "sqrt_recip_alpha_bar_minus_one")}


def normalize_mel(mel):
    mean = mel.mean(dim=1, keepdim=True)
    std = mel.std(dim=1, keepdim=True).clamp_min(1e-5)
    return (mel - mean) / std, mean, std


def _co(tab, t):
    return tuple(tab[n][t].reshape(-1, 1, 1) for n in ("sqrt_alpha_bar", "sqrt_one_minus_alpha_bar", "sqrt_recip_alpha_bar", "sqrt_recip_alpha_bar_minus_one"))


def _losses(kind, tab, mel_n, noise, x_t, t, t2, p, p2):
    """The reference's expressions on tensors already aligned to one length: (squared-error sums of the loss's terms, x0, x0 of the
    metrics' comparison).  The caller divides by the element count."""
    sab, s1m, sra, srm1 = _co(tab, t)
    if kind == "v":
        target = sab * noise - s1m * mel_n                                   # get_v_target
        x0 = sab * x_t - s1m * p                                             # predict_x0_from_v
        return [((p - target) ** 2).sum()], x0
    if kind == "eps":
        x0 = sra * x_t - srm1 * p                                            # predict_x0_from_eps
        return [((p - noise) ** 2).sum()], x0
    if kind == "distill":                                                    # consistency.py:77-83
        x0 = sab * x_t - s1m * p
        x0_t = sab * x_t - s1m * p2.detach()
        return [((x0 - x0_t) ** 2).sum()], x0
    sab2, s1m2, _, _ = _co(tab, t2)                                          # consistency.py:101-120
    x_t2 = sab2 * mel_n + s1m2 * noise
    x0 = sab * x_t - s1m * p
    x0_2 = sab2 * x_t2 - s1m2 * p2
    return [((x0 - x0_2.detach()) ** 2).sum(), ((x0 - mel_n) ** 2).sum(), ((x0_2 - mel_n) ** 2).sum()], x0


def _tm(kind, T, Tp, Tp2):
    return min(T, Tp, Tp2) if kind in ("distill", "consistency") else min(T, Tp)


def _finish(kind, sums, n, mse_sum, cos, pred, pred2, extra):
    terms = [s / n for s in sums]
    loss = terms[0] + 0.5 * (terms[1] + terms[2]) if kind == "consistency" else terms[0]
    loss.backward()
    out = dict(extra, loss=loss.detach(), terms=torch.stack([t.detach() for t in terms]), d_pred=pred.grad, x0_mse=mse_sum / n,
               x0_cos=torch.cat(cos).mean())
    if kind == "consistency":
        out["d_pred2"] = pred2.grad
    return out


def _leaves(inp, dtype, pred_of, x_t):
    """(pred, pred2) as leaves of the graph -- or pred = pred_of(x_t), the prediction of a decoder whose parameters are the leaves."""
    if pred_of is None:
        pred = inp["pred"].to(dtype).clone().requires_grad_(True)
    else:
        pred = pred_of(x_t)
        pred.retain_grad()
    return pred, inp["pred2"].to(dtype).clone().requires_grad_(True)


def _normalize(mel, normalize):
    return normalize_mel(mel) if normalize else (mel, torch.zeros_like(mel[:, :1]), torch.ones_like(mel[:, :1]))


def padded(inp, kind, dtype, pred_of=None, normalize=True):
    """The batch expression of the reference: statistics, means and cosine over all T frames (train_v2.py:112-154)."""
    tab = tables(dtype)
    mel, noise = inp["mel"].to(dtype), inp["noise"].to(dtype)
    mel_n, mean, std = _normalize(mel, normalize)
    sab, s1m, _, _ = _co(tab, inp["t"])
    x_t = sab * mel_n + s1m * noise                                          # q_sample
    target = noise if kind == "eps" else sab * noise - s1m * mel_n
    pred, pred2 = _leaves(inp, dtype, pred_of, x_t)
    tm = _tm(kind, mel.shape[1], pred.shape[1], pred2.shape[1])
    a = lambda v: v[:, :tm]
    sums, x0 = _losses(kind, tab, a(mel_n), a(noise), a(x_t), inp["t"], inp["t2"], a(pred), a(pred2))
    n = mel.shape[0] * tm * mel.shape[2]
    with torch.no_grad():
        mse = ((x0 - a(mel_n)) ** 2).sum()
        cos = [F.cosine_similarity(x0.flatten(1), a(mel_n).flatten(1), dim=1)]
    return _finish(kind, sums, n, mse, cos, pred, pred2, dict(mean=mean, std=std, x_t=x_t, target=target))


def ragged(inp, kind, dtype, lengths=None, pred_of=None, normalize=True):
    """Every row trimmed to its length and evaluated alone; x_t and target come back padded with zeros."""
    tab = tables(dtype)
    mel, noise = inp["mel"].to(dtype), inp["noise"].to(dtype)
    B, T, M = mel.shape
    lengths = [int(v) for v in (inp["lengths"] if lengths is None else lengths)]
    rows, means, stds = [], [], []
    x_t_all, target_all = torch.zeros_like(mel), torch.zeros_like(mel)
    for b, L in enumerate(lengths):
        mel_n, mean, std = _normalize(mel[b:b + 1, :L], normalize)
        nz, t = noise[b:b + 1, :L], inp["t"][b:b + 1]
        sab, s1m, _, _ = _co(tab, t)
        x_t = sab * mel_n + s1m * nz
        x_t_all[b, :L], target_all[b, :L] = x_t[0], (nz if kind == "eps" else sab * nz - s1m * mel_n)[0]
        means.append(mean)
        stds.append(std)
        rows.append((mel_n, nz, x_t, t, inp["t2"][b:b + 1]))
    pred, pred2 = _leaves(inp, dtype, pred_of, x_t_all)
    tm = _tm(kind, T, pred.shape[1], pred2.shape[1])
    n = sum(min(L, tm) for L in lengths) * M
    sums, mse, cos = None, 0.0, []
    for b, (L, (mel_n, nz, x_t, t, t2)) in enumerate(zip(lengths, rows)):
        l = min(L, tm)
        a = lambda v: v[:, :l]
        s, x0 = _losses(kind, tab, a(mel_n), a(nz), a(x_t), t, t2, pred[b:b + 1, :l], pred2[b:b + 1, :l])
        sums = s if sums is None else [u + v for u, v in zip(sums, s)]
        with torch.no_grad():
            mse = mse + ((x0 - a(mel_n)) ** 2).sum()
            cos.append(F.cosine_similarity(x0.flatten(1), a(mel_n).flatten(1), dim=1))
    return _finish(kind, sums, n, mse, cos, pred, pred2, dict(mean=torch.cat(means), std=torch.cat(stds), x_t=x_t_all, target=target_all))


# ---------------------------------------------------------------------------------------------- the chain with the decoder
def chain_inputs(name):
    """(cfg, state dict, decoder inputs, frame lengths, token lengths, objective inputs) of a composition case: a case of
    tests/train_util.py (padded) or tests/train_ragged_util.py (ragged).  Its x is the mel, its target the injected noise."""
    import train_ragged_util
    import train_util
    if name in train_util.CASES:
        cfg, sd, inp = train_util.case(name)
        t_len = s_len = None
    else:
        cfg, sd, inp, t_len, s_len = train_ragged_util.case(name)
    B, T, M = inp["x"].shape
    oinp = dict(mel=inp["x"], noise=inp["target"], t=inp["t"], t2=inp["t"], pred2=torch.zeros(B, T, M))
    return cfg, sd, inp, t_len, s_len, oinp


def chain_grads(name, dtype):
    """(loss, {parameter name | "d_sem_features": gradient}) of oracle decoder + oracle objective ("v") under torch.autograd: the
    padded forms for a padded case (with normalize_mel), the per-utterance forms for a ragged one (mel taken as normalised: a
    one-frame row has no std)."""
    import train_ragged_util
    from oracle import edtts_oracle as O
    from train_util import BUFFERS
    cfg, sd, inp, t_len, s_len, oinp = chain_inputs(name)
    p = {k: (v.to(dtype).clone().requires_grad_(k not in BUFFERS) if v.is_floating_point() else v) for k, v in sd.items()}
    f = None if inp["f"] is None else inp["f"].to(dtype).clone().requires_grad_(True)
    if t_len is None:
        out = padded(oinp, "v", dtype, pred_of=lambda x_t: O.decoder_forward(p, x_t, inp["t"], inp["sem"], inp["si"], f, heads=cfg.heads,
                                                                             window=cfg.attn_window_size))
    else:
        def pred_of(x_t):
            eps = train_ragged_util.ragged_eps(cfg, p, x_t, f, inp, t_len, s_len)
            return torch.cat([F.pad(e, (0, 0, 0, x_t.shape[1] - e.shape[1])) for e in eps])
        out = ragged(oinp, "v", dtype, lengths=t_len, pred_of=pred_of, normalize=False)
    grads = {k: v.grad for k, v in p.items() if v.is_floating_point() and k not in BUFFERS}
    if f is not None:
        grads["d_sem_features"] = f.grad
    return out["loss"], grads


@functools.lru_cache(maxsize=None)
def chain_pair(name):
    """(fp64 gradients, E_ref per tensor, median E_ref, fp64 loss) of a composition case, computed once."""
    from train_util import rel_err
    l64, g64 = chain_grads(name, torch.float64)
    _, g32 = chain_grads(name, torch.float32)
    e_ref = {k: rel_err(g32[k], g64[k]) for k in g64 if g64[k] is not None}
    return g64, e_ref, float(torch.tensor(sorted(e_ref.values())).median()), l64


@functools.lru_cache(maxsize=None)
def pair(name, kind, with_lengths=True):
    """(fp64 oracle, fp32 oracle) of a case: the ragged form with the case's lengths, or the padded form."""
    inp = case(name)
    if with_lengths:
        return ragged(inp, kind, torch.float64), ragged(inp, kind, torch.float32)
    return padded(inp, kind, torch.float64), padded(inp, kind, torch.float32)


def error(got, ref64):
    """E = max|got - ref| / max|ref| (a scalar: its relative error)."""
    got, ref64 = got.detach().cpu().double(), ref64.double()
    return float((got - ref64).abs().max() / ref64.abs().max())


def reference_errors(o64, o32, names):
    """E_ref of every quantity: the fp32 oracle's error; for a scalar floored at one fp32 ulp of the fp64 value."""
    out = {}
    for k in names:
        e = error(o32[k], o64[k])
        if o64[k].dim() == 0:
            v = abs(float(o64[k]))
            e = max(e, float(np.spacing(np.float32(v))) / v)
        out[k] = e
    return out


def check(got, o64, o32, what, scale=None):
    """Every entry of `got` within MARGIN * max(E_ref, median E_ref) of the fp64 oracle; ``scale``: {name: factor on the oracle's
    value}.  Prints each figure and returns the worst ratio."""
    e_ref = reference_errors(o64, o32, list(got))
    med = float(np.median(sorted(e_ref.values())))
    worst, bad = 0.0, []
    for k, v in got.items():
        ref = o64[k] * (scale or {}).get(k, 1.0)
        assert tuple(v.shape) == tuple(ref.shape), (k, tuple(v.shape), tuple(ref.shape))
        assert float(ref.abs().max()) > 0, f"{what}: {k} is all zero in the fp64 oracle (a vacuous comparison)"
        e, bar = error(v, ref), max(e_ref[k], med)
        print(f"{what} {k}: E {e:.2e}  E_ref {e_ref[k]:.2e}  ratio {e / bar:.2f}")
        worst = max(worst, e / bar)
        if not e <= MARGIN * bar:
            bad.append((k, e, e_ref[k], med))
    print(f"{what}: worst ratio {worst:.2f} (median E_ref {med:.2e})")
    assert not bad, bad
    return worst


def frame_mask(lengths, T):
    """[B, T, 1] bool: frame i of row b is live."""
    return (torch.arange(T, device=lengths.device)[None, :] < lengths[:, None])[..., None]
