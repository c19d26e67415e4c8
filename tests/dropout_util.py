"""Shared by tests/test_dropout_host.py, tests/test_dropout_gpu.py and tests/golden/make_golden_dropout.py: the dropout mask
contract of include/edtts.h ("Dropout masks") restated in numpy -- from the contract's text, not from the kernels -- and the CPU
oracle with the four masks applied where the reference applies dropout.

Contract: thr = round(p * 65536), p_eff = thr / 65536, an element is kept iff its 16-bit field >= thr, kept values are multiplied by
1 / (1 - p_eff).  One draw = Philox4x32-10(key = (seed lo, seed hi), counter = (c0, c1, c2, c3)) = eight 16-bit fields, field j =
bits [16 (j & 1), +16) of output word j >> 1.  c2 = 0x30000 + 4 layer + site.  Sites 0 / 1 (attention probabilities of utterance b,
head h, query q, key k): c0 = k >> 2, c1 = q >> 1, c3 = b heads + h, field 4 (q & 1) + (k & 3).  Sites 2 / 3 (row m = b T + t,
column n of the SwiGLU output / the down projection): c0 = n >> 3, c1 = m, c3 = 0, field n & 7."""
import functools

import numpy as np
import torch

from oracle import edtts_oracle as O
from train_util import BUFFERS, case, rel_err

SITE_ATTN, SITE_CROSS, SITE_ACT, SITE_DOWN = 0, 1, 2, 3
_MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(key, counter):
    """Philox4x32-10 (Salmon et al., SC'11).  key: 2 words, counter: 4 words (ints or broadcastable arrays) -> 4 uint64 arrays
    holding the 32-bit output words."""
    k0, k1 = (np.asarray(v, dtype=np.uint64) for v in key)
    c0, c1, c2, c3 = (np.asarray(v, dtype=np.uint64) for v in counter)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0  # (32 x 32 bits: no overflow in 64)
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ k0) & _MASK32, p1 & _MASK32, ((p0 >> np.uint64(32)) ^ c3 ^ k1) & _MASK32, p0 & _MASK32
        k0 = (k0 + np.uint64(0x9E3779B9)) & _MASK32
        k1 = (k1 + np.uint64(0xBB67AE85)) & _MASK32
    return c0, c1, c2, c3


def threshold(p):
    """round(p * 65536) of the fp32 value the C ABI carries (EdttsDropout.p is a float)."""
    thr = int(round(float(np.float32(p)) * 65536.0))
    if not (0.0 <= p < 1.0) or thr > 65535:
        raise ValueError(f"p={p} outside the contract's range")
    return thr


def scale(p):
    """1 / (1 - p_eff)."""
    return 65536.0 / (65536.0 - threshold(p))


def field(words, j):
    """Field j (array, 0 .. 7) of a draw's four words."""
    j = np.asarray(j)
    w = np.choose(j >> 1, np.broadcast_arrays(*words))
    return (w >> (np.uint64(16) * (j & 1).astype(np.uint64))) & np.uint64(0xFFFF)


def stream_word(layer, site):
    return 0x30000 + 4 * layer + site


def _key(seed):
    return seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF


def attn_keep(seed, p, layer, site, B, heads, Tq, Tk):
    """bool [B, heads, Tq, Tk]: the keep mask of the attention probabilities (site 0: Tk = T, site 1: Tk = S)."""
    bh = np.arange(B * heads, dtype=np.int64).reshape(B, heads, 1, 1)
    q = np.arange(Tq, dtype=np.int64).reshape(1, 1, Tq, 1)
    k = np.arange(Tk, dtype=np.int64).reshape(1, 1, 1, Tk)
    words = philox4x32_10(_key(seed), (k >> 2, q >> 1, stream_word(layer, site), bh))
    return field(words, 4 * (q & 1) + (k & 3) + 0 * bh) >= threshold(p)


def row_keep(seed, p, layer, site, rows, width):
    """bool [rows, width]: the keep mask behind SwiGLU (site 2, width ffn_mult * hidden) / behind ffn.net.3 (site 3, width hidden)."""
    m = np.arange(rows, dtype=np.int64).reshape(rows, 1)
    n = np.arange(width, dtype=np.int64).reshape(1, width)
    words = philox4x32_10(_key(seed), (n >> 3, m, stream_word(layer, site), 0))
    return field(words, (n & 7) + 0 * m) >= threshold(p)


def multiplier(keep, p, dtype):
    """keep * 1 / (1 - p_eff) as a tensor of `dtype`."""
    return torch.from_numpy(np.ascontiguousarray(keep)).to(dtype) * torch.tensor(scale(p), dtype=dtype)


# --------------------------------------------------------------------------------------------------- the masked oracle
def _attention(q, k, v, mask, mult):
    s = (q @ k.transpose(-1, -2)) * (q.shape[-1] ** -0.5)
    if mask is not None:
        s = s.masked_fill(~mask, float("-inf"))
    a = torch.softmax(s, dim=-1)
    if mult is not None:
        a = a * mult  # layers/attention.py:117-119, layers/mla.py:188-190: dropout(softmax(s)) @ v
    return a @ v


def decoder_forward(sd, x_t, t, sem_idx=None, step_idx=None, sem_features=None, *, heads, window, p=0.0, seed=0):
    """oracle.edtts_oracle.decoder_forward from the same pieces in the same order, with the masks of (p, seed) at the reference's
    four dropout sites; p = 0: no mask is applied and the result is that function's, exactly."""
    cond = O.time_condition(sd, t, step_idx)
    ctx = O.context_embed(sd, sem_idx, sem_features)
    h = O.input_embed(sd, x_t)
    B, T, H = h.shape
    S = ctx.shape[1]

    def mult(l, site):
        if p == 0:
            return None
        if site == SITE_ATTN:
            return multiplier(attn_keep(seed, p, l, site, B, heads, T, T), p, h.dtype)
        if site == SITE_CROSS:
            return multiplier(attn_keep(seed, p, l, site, B, heads, T, S), p, h.dtype)
        width = sd[f"layers.{l}.ffn.net.3.weight"].shape[1] if site == SITE_ACT else H
        return multiplier(row_keep(seed, p, l, site, B * T, width), p, h.dtype).reshape(B, T, width)

    for l in range(O.n_layers(sd)):
        pre = f"layers.{l}."
        # layers/attention.py:77-123
        qkv = O.linear(O.ada_rms_norm(h, cond, sd, pre + "norm1."), sd[pre + "attn.qkv.weight"])
        q, k, v = (O.split_heads(qkv[..., i * H:(i + 1) * H], heads) for i in range(3))
        band = O.band_mask(T, window) if window is not None else None
        a = _attention(q, k, v, band, mult(l, SITE_ATTN))
        h = h + O.linear(O.merge_heads(a), sd[pre + "attn.proj.weight"], sd[pre + "attn.proj.bias"])
        # layers/mla.py:118-194 (cross mode)
        q = O.split_heads(O.linear(O.rms_norm(h, sd[pre + "norm2.weight"]), sd[pre + "cross_attn.q_proj.weight"]), heads)
        k, v = O.cross_kv(sd, pre + "cross_attn.", ctx, heads)
        a = _attention(q, k, v, None, mult(l, SITE_CROSS))
        h = h + O.linear(O.merge_heads(a), sd[pre + "cross_attn.out_proj.weight"])
        # layers/transformer.py:13-49
        u = O.linear(O.ada_rms_norm(h, cond, sd, pre + "norm3."), sd[pre + "ffn.net.0.weight"], sd[pre + "ffn.net.0.bias"])
        half = u.shape[-1] // 2
        val, gate = u[..., :half], u[..., half:]
        act = val * (gate * torch.sigmoid(gate))
        m2, m3 = mult(l, SITE_ACT), mult(l, SITE_DOWN)
        if m2 is not None:
            act = act * m2
        y = O.linear(act, sd[pre + "ffn.net.3.weight"], sd[pre + "ffn.net.3.bias"])
        if m3 is not None:
            y = y * m3
        h = h + y
    return O.linear(O.layer_norm(h, sd["final_norm.weight"], sd["final_norm.bias"]), sd["out_proj.weight"], sd["out_proj.bias"])


def oracle_grads(cfg, sd, inp, dtype, p, seeds, two=False, loss_fn=None):
    """train_util.oracle_grads on the masked oracle: forward i runs with seeds[i].  Returns (loss, gradients, eps of forward 0)."""
    prm = {k: (v.to(dtype).clone().requires_grad_(k not in BUFFERS) if v.is_floating_point() else v) for k, v in sd.items()}
    x = inp["x"].to(dtype).clone().requires_grad_(True)
    f = None if inp["f"] is None else inp["f"].to(dtype).clone().requires_grad_(True)
    calls = []

    def fwd(t):
        out = decoder_forward(prm, x, t, inp["sem"], inp["si"], f, heads=cfg.heads, window=cfg.attn_window_size, p=p, seed=seeds[len(calls)])
        calls.append(out.detach())
        return out

    if loss_fn is not None:
        loss = loss_fn(fwd, x)
    else:
        loss = ((fwd(inp["t"]) - inp["target"].to(dtype)) ** 2).mean()
        if two:
            loss = loss + ((fwd(inp["t2"]) - inp["target2"].to(dtype)) ** 2).mean()
    loss.backward()
    grads = {k: v.grad for k, v in prm.items() if v.is_floating_point() and k not in BUFFERS}
    grads["d_x"] = x.grad
    if f is not None:
        grads["d_sem_features"] = f.grad
    return loss.detach(), grads, calls[0]


@functools.lru_cache(maxsize=None)
def oracle_pair(name, p, seeds, two=False):
    """(fp64 gradients, E_ref per tensor, median E_ref, fp32 eps of forward 0) of a train_util case under the masks of (p, seeds)."""
    cfg, sd, inp = case(name)
    _, g64, _ = oracle_grads(cfg, sd, inp, torch.float64, p, seeds, two)
    _, g32, eps32 = oracle_grads(cfg, sd, inp, torch.float32, p, seeds, two)
    e_ref = {k: rel_err(g32[k], g64[k]) for k in g64 if g64[k] is not None}
    return g64, e_ref, float(torch.tensor(sorted(e_ref.values())).median()), eps32


def seeds_of(generator_seed, n=1):
    """The first n 63-bit seeds a decoder with dropout_generator = torch.Generator().manual_seed(generator_seed) draws."""
    g = torch.Generator().manual_seed(generator_seed)
    return tuple(int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64, generator=g).item()) for _ in range(n))
