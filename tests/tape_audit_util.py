"""Shared by tests/test_tape_audit_host.py and tests/test_tape_audit_gpu.py: the stage-by-stage audit of the generic training forward
(DESIGN.md section 29).  After one edtts_decoder_forward_train the caller-owned tape holds the inputs AND the output of almost every
launch of GenericLauncher::ctx / ::forward, so each launch is compared element by element with an fp64 evaluation of the same operands
under the rounding contract of include/edtts.h (EDTTS_MATMUL_BF16, EDTTS_ATTN_BF16, EDTTS_TAPE_BF16): only MFMA operands are rounded,
bf16 x bf16 products are exact in fp32, everything else is fp32.  The bars are sums of derived terms (u = 2^-24):

  accumulation  K u sum_k |a_k||w_k| per GEMM (any summation order of exact products), 2 u |partial| per epilogue add or multiply
  norm class    the kernel rounds an fp32 norm row to bf16, the reference an fp64 one: with d = ETA x (the summands' magnitudes),
                lo = rnd(xn - d) and hi = rnd(xn + d) bracket the kernel's operand; elements with lo != hi ("ambiguous") add
                |hi - lo||w| to their row's bar.  Without rounding the term is d |w| over all k.
  attention     LSE: max_j dS_ij + (n_i + C_LSE) u max(1, |LSE|), dS_ij = d u sum|q||k| / sqrt(d), n_i live keys
                O: (2^-8 [bf16 attention] + (n_i + 2) u) sum_j p_j D_j |V_jd| + LSE bar x |O|
  function      C_FN u |value silu(gate)| for the SwiGLU sigmoid
  storage       a region narrowed by EDTTS_TAPE_BF16 adds half a bf16 ulp to its producer's bar; consumers read exact operands

ETA, C_LSE and C_FN are train_util.MARGIN times the fp32 CPU oracle's own worst error against fp64 on the audit cases (measured by
measure_allowances, asserted by the host test).  Nothing here is fitted to what the kernels give.

A "tape" below is a dict of fp64 tensors shaped as the tape's regions: tcond, cond, ctx, hl, eps and layers[l][region]."""
import collections
import functools
import math

import torch

import attn_bf16_util as AU
import dropout_util as DU
import train_ragged_util as R
from edge_diffusion_tts_amd import CFG, synth_state_dict
from oracle import edtts_oracle as O
from train_util import MARGIN

F64, F32 = torch.float64, torch.float32
u = 2.0 ** -24
LN2 = math.log(2.0)

# MARGIN x the fp32 oracle's worst error (measure_allowances; tests/test_tape_audit_host.py asserts that they still are)
ETA = 2.0 ** -19     # norm rows, relative to |rms_norm(x) w||1 + scale| + |shift| (LayerNorm: (|x| + |mean|) rstd |w| + |b|)
C_LSE = 16.0         # exp / log of the log-sum-exp, in units of u max(1, |LSE|)
C_FN = 16.0          # g sigmoid(g), in units of u |g sigmoid(g)|
AMBIGUOUS_MAX = 0.01  # the norm-class argument needs the bracket to be decided for all but 1 % of any stage's operand

Opts = collections.namedtuple("Opts", "mm att tape")  # matmul_dtype, attn_dtype, tape_dtype == "bf16"
OPTION_SETS = (Opts(False, False, False), Opts(True, False, False), Opts(False, True, False), Opts(True, True, False), Opts(True, True, True))

# the head-dim sweep: k_gen_attn16<DT> for DT = 4 .. 7 (layers = 1, B = 2); (cfg keywords, B, T, S, features, step_idx) as train_util.CASES
DCASES = {
    "D4": (dict(hidden=112, heads=2, attn_window_size=7, layers=1), 2, 70, 33, True, True),                     # head_dim 56: DT 4, KS 2
    "D5": (dict(hidden=144, heads=2, attn_window_size=None, layers=1, codebook_size=16), 2, 65, 32, False, True),  # 72: DT 5, KS 3; ids
    "D6": (dict(hidden=180, heads=2, attn_window_size=40, layers=1), 2, 97, 70, True, True),                    # 90: DT 6, scalar loaders
    "D7": (dict(hidden=208, heads=2, attn_window_size=0, layers=1), 2, 64, 1, True, True),                      # 104: DT 7, KS 4; one key
}
# ragged: R2 is train_ragged_util's; R4 is new HERE (that module's own R4 is another case): A1's configuration with a dead third
# 64-query block (17), a block with one live query (65) and a block with one live wave plus one row (17 = 16 + 1)
R4 = ("A1", 3, 130, 70, (130, 65, 17), (70, 33, 5))
PLAIN = ("G1", "G2", "G3", "G4", "G5", "A1", "A2", "D4", "D5", "D6", "D7")
RAGGED = ("R2", "R4")
DROPPED = ("G2", "D5")

Case = collections.namedtuple("Case", "name cfg sd inp B T S t_len s_len")


def _draw(cfg, B, T, S, feats, with_step, seed):
    g = torch.Generator().manual_seed(seed)
    return dict(x=torch.randn(B, T, cfg.n_mels, generator=g), t=torch.randint(0, 1000, (B,), generator=g),
                si=torch.randint(0, 16, (B,), generator=g) if with_step else None,
                sem=None if feats else torch.randint(0, cfg.codebook_size, (B, S), generator=g),
                f=torch.randn(B, S, cfg.semantic_dim, generator=g) if feats else None)


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "R2":
        cfg, sd, inp, t_len, s_len = R.case(name)
        return Case(name, cfg, sd, inp, *inp["x"].shape[:2], int(s_len.max()), t_len, s_len)
    if name == "R4":
        base, B, T, S, t_len, s_len = R4
        kw, _, _, _, feats, with_step = AU.ACASES[base]
        cfg = CFG(device="cpu", **kw)
        return Case(name, cfg, synth_state_dict(cfg, 0), _draw(cfg, B, T, S, feats, with_step, B * 1000 + T + 7), B, T, S,
                    torch.tensor(t_len), torch.tensor(s_len))
    if name in DCASES:
        kw, B, T, S, feats, with_step = DCASES[name]
        cfg = CFG(device="cpu", **kw)
        return Case(name, cfg, synth_state_dict(cfg, 0), _draw(cfg, B, T, S, feats, with_step, B * 1000 + T), B, T, S, None, None)
    cfg, sd, inp = AU.case(name)
    return Case(name, cfg, sd, inp, *AU.shape(name), None, None)


# ------------------------------------------------------------------------------------------------------------ small pieces
def bf16(v):
    """Round to nearest even to bf16 (through fp32: every operand the kernels round is an fp32 value)."""
    return v.to(F32).to(torch.bfloat16).to(v.dtype)


def ident(v):
    return v


def half_ulp_bf16(v):
    """Half the spacing of bf16 at |v| (8 significant bits)."""
    _, e = torch.frexp(v.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(v), e - 9)


def gemm(a, w, rnd):
    """(rnd(a) rnd(w)^T, K u |rnd(a)||rnd(w)|^T)."""
    a, w = rnd(a), rnd(w)
    return a @ w.T, (a.shape[-1] * u) * (a.abs() @ w.abs().T)


def adds(*partials):
    """2 u |partial| per epilogue add / multiply: `partials` are the exact results of those operations."""
    return sum(2 * u * p.abs() for p in partials)


def rms_rows(x, w, eps=1e-6):
    return x * torch.rsqrt(x.pow(2).mean(dim=-1, keepdim=True) + eps) * w


def ada_rows(x, w, mod):
    """(AdaLN row, its uncertainty d).  mod [rows][2H] = (1 + scale | shift), or None: the plain RMSNorm."""
    y = rms_rows(x, w)
    if mod is None:
        return y, ETA * y.abs()
    H = x.shape[-1]
    return y * mod[:, :H] + mod[:, H:], ETA * (y.abs() * mod[:, :H].abs() + mod[:, H:].abs())


def layer_rows(x, w, b, eps=1e-5):
    mu = x.mean(dim=-1, keepdim=True)
    rs = torch.rsqrt((x - mu).pow(2).mean(dim=-1, keepdim=True) + eps)
    return (x - mu) * rs * w + b, ETA * ((x.abs() + mu.abs()) * rs * w.abs() + b.abs())


def normed_gemm(xn, d, w, rnd, on, amb=None, live=None):
    """The norm class: a GEMM whose left operand the kernel computed itself in fp32 (xn +- d bounds it).  amb: a list that receives
    the stage's ambiguous fraction (of the live rows)."""
    wr = rnd(w)
    if on:
        lo, hi = rnd(xn - d), rnd(xn + d)
        if amb is not None:
            amb.append(float((lo != hi)[slice(None) if live is None else live].double().mean()))
        a, extra = rnd(xn), (hi - lo).abs() @ wr.abs().T
    else:
        a, extra = xn, d @ wr.abs().T
    return a @ wr.T, (a.shape[-1] * u) * (a.abs() @ wr.abs().T) + extra


def key_mask(T, Tk, window, k_len, B):
    """[B, 1, T, Tk] bool: key j is read by query i (band and per-utterance key count)."""
    ok = torch.ones(T, Tk, dtype=torch.bool) if window is None else (torch.arange(Tk)[None, :] - torch.arange(T)[:, None]).abs() <= window
    ok = ok[None, None].expand(B, 1, T, Tk)
    if k_len is not None:
        ok = ok & (torch.arange(Tk)[None, :] < k_len[:, None])[:, None, None, :]
    return ok


def live_keys(k, k_len):
    """Rows at or past an utterance's key count are never loaded: zero (the padding may hold NaN)."""
    if k_len is None:
        return k
    return torch.where((torch.arange(k.shape[1])[None, :] < k_len[:, None])[..., None], k, torch.zeros_like(k))


def attention(q, k, v, heads, window, k_len, rnd, att16, mult):
    """q [B, T, H], k / v [B, Tk, H] -> (O [B, T, H], its bar, natural LSE [B, heads, T], its bar).  mult: the dropout multiplier
    [B, heads, T, Tk] or None; the LSE is the undropped one."""
    B, T, H = q.shape
    Tk, d = k.shape[1], H // heads
    qh, kh, vh = (O.split_heads(rnd(z), heads) for z in (q, live_keys(k, k_len), live_keys(v, k_len)))
    ok = key_mask(T, Tk, window, k_len, B)
    s = ((qh @ kh.transpose(-1, -2)) / math.sqrt(d)).masked_fill(~ok, float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse[..., None])
    n = ok.sum(dim=-1).to(F64).expand(B, heads, T)
    ds = ((d * u / math.sqrt(d)) * (qh.abs() @ kh.abs().transpose(-1, -2))).masked_fill(~ok, 0.0).amax(dim=-1)
    lse_bar = ds + (n + C_LSE) * u * lse.abs().clamp_min(1.0)
    pd = p if mult is None else p * mult
    o = pd @ vh
    o_bar = ((2.0 ** -8 if att16 else 0.0) + (n + 2) * u)[..., None] * (pd @ vh.abs()) + lse_bar[..., None] * o.abs()
    return O.merge_heads(o), O.merge_heads(o_bar), lse, lse_bar


def swiglu(uu, uu_bar, mult):
    """value * silu(gate) (* dropout multiplier) of the biased up projection and the bar that its bar becomes."""
    half = uu.shape[-1] // 2
    v, g, ev, eg = uu[:, :half], uu[:, half:], uu_bar[:, :half], uu_bar[:, half:]
    sg = torch.sigmoid(g)
    silu, dsilu = g * sg, (sg * (1 + g * (1 - sg))).abs() + 0.5 * eg  # (|silu''| <= 1/2)
    act = v * silu
    bar = silu.abs() * ev + v.abs() * dsilu * eg + dsilu * ev * eg + (C_FN * u + 2 * u) * act.abs()
    if mult is not None:
        act, bar = act * mult, bar * mult + adds(act * mult)
    return act, bar


# ------------------------------------------------------------------------------------------------------------ the walk
def weights(cs):
    return O.cast_sd(cs.sd, F64)


def drop_mults(cs, p, seed):
    """{(layer, site): multiplier} from dropout_util's restatement of the mask contract."""
    B, T, S, cfg = cs.B, cs.T, cs.S, cs.cfg
    out = {}
    for l in range(cfg.layers):
        out[l, 0] = DU.multiplier(DU.attn_keep(seed, p, l, 0, B, cfg.heads, T, T), p, F64)
        out[l, 1] = DU.multiplier(DU.attn_keep(seed, p, l, 1, B, cfg.heads, T, S), p, F64)
        out[l, 2] = DU.multiplier(DU.row_keep(seed, p, l, 2, B * T, cfg.ffn_mult * cfg.hidden), p, F64)
        out[l, 3] = DU.multiplier(DU.row_keep(seed, p, l, 3, B * T, cfg.hidden), p, F64)
    return out


def row_mask(lens, B, n):
    """[B n] bool: row b n + i is live."""
    return torch.ones(B * n, dtype=torch.bool) if lens is None else (torch.arange(n)[None, :] < lens[:, None]).reshape(-1)


def stages(cs, opts, tp, drop=None, amb=None):
    """Yields (name, class, reference, bar, live mask or None, where the output lies) for every audited launch, in launch order,
    each from the operands that `tp` holds at that moment: a caller that stores the reference before asking for the next stage chains
    the references; one that holds a filled tape audits it.  `where`: (layer or None, region)."""
    cfg, sd, inp, B, T, S = cs.cfg, weights(cs), cs.inp, cs.B, cs.T, cs.S
    H, heads, L = cfg.hidden, cfg.heads, cfg.layers
    r_mm, r_at = (bf16 if opts.mm else ident), (bf16 if opts.att else ident)
    frames, toks = row_mask(cs.t_len, B, T), row_mask(cs.s_len, B, S)
    fh = frames.reshape(B, 1, T).expand(B, heads, T).reshape(B * heads, T)  # the log-sum-exps' layout
    dm = drop or {}

    def narrowed(ref, bar):
        return bar + half_ulp_bf16(ref.abs() + bar) if opts.tape else bar

    # 0a context rows
    pe = sd["context_pos_emb.pe"][:S].repeat(B, 1)
    if inp["f"] is not None:
        y, bar = gemm(inp["f"].to(F64).reshape(B * S, -1), sd["sem_proj.weight"], r_mm)
        yb = y + sd["sem_proj.bias"]
        ref, bar = yb + pe, bar + adds(yb, yb + pe)
    else:
        tok = sd["token_emb.weight"][inp["sem"].reshape(-1)]
        ref, bar = tok + pe, adds(tok + pe)
    yield "ctx", "exact", ref, bar, toks, (None, "ctx")
    # c AdaLN rows (1 + scale | shift) of every layer: norm1 then norm3
    refs, bars = [], []
    for l in range(L):
        for nm in ("norm1.", "norm3."):
            pw = sd.get(f"layers.{l}.{nm}proj.weight")
            if pw is None:  # plain RMSNorm blocks: the modulation slots hold zeros
                pw, pb = torch.zeros(2 * H, H, dtype=F64), torch.zeros(2 * H, dtype=F64)
            else:
                pb = sd[f"layers.{l}.{nm}proj.bias"]
            y, bar = gemm(tp["tcond"], pw, r_mm)
            yb = y + pb
            one = torch.cat([torch.ones(H, dtype=F64), torch.zeros(H, dtype=F64)])
            refs.append(yb + one)
            bars.append(bar + adds(yb, (yb + one) * one))
    ref = torch.stack(refs, 1).reshape(B * L * 2, 2 * H)
    yield "cond", "exact", ref, torch.stack(bars, 1).reshape(B * L * 2, 2 * H), None, (None, "cond")
    cond = tp["cond"].reshape(B, L, 2, 2 * H)
    adaln = "layers.0.norm1.proj.weight" in sd

    def mod(l, which):
        return cond[:, l, which].repeat_interleave(T, 0) if adaln else None

    def gain(l, nm):
        return sd[f"layers.{l}.{nm}.norm.weight"] if adaln else sd[f"layers.{l}.{nm}.weight"]

    # 1, 2 the cross K|V rows of every layer (GenericLauncher::ctx runs before the blocks)
    for l in range(L):
        z, p = tp["layers"][l], f"layers.{l}.cross_attn."
        ref, bar = gemm(tp["ctx"], sd[p + "kv_down_proj.weight"], r_mm)
        yield f"L{l}.crp", "exact", ref, bar, toks, (l, "crp")
        xn = rms_rows(z["crp"], sd[p + "kv_norm.weight"])
        ref, bar = normed_gemm(xn, ETA * xn.abs(), sd[p + "kv_up_proj.weight"], r_mm, opts.mm, amb, toks)
        yield f"L{l}.kv", "norm", ref, narrowed(ref, bar), toks, (l, "kv")
    # 0b the residual stream entering layer 0
    y, bar = gemm(inp["x"].to(F64).reshape(B * T, -1), sd["in_proj.weight"], r_mm)
    yb, pe = y + sd["in_proj.bias"], sd["pos_emb.pe"][:T].repeat(B, 1)
    yield "L0.h0", "exact", yb + pe, bar + adds(yb, yb + pe), frames, (0, "h0")
    for l in range(L):
        z, p = tp["layers"][l], f"layers.{l}."
        # 3 q|k|v
        xn, d = ada_rows(z["h0"], gain(l, "norm1"), mod(l, 0))
        ref, bar = normed_gemm(xn, d, sd[p + "attn.qkv.weight"], r_mm, opts.mm, amb, frames)
        yield f"L{l}.qkv", "norm", ref, narrowed(ref, bar), frames, (l, "qkv")
        # 4 self-attention
        q, k, v = (z["qkv"][:, i * H:(i + 1) * H].reshape(B, T, H) for i in range(3))
        o, o_bar, lse, lse_bar = attention(q, k, v, heads, cfg.attn_window_size, cs.t_len, r_at, opts.att, dm.get((l, 0)))
        yield f"L{l}.att1", "attention", o.reshape(B * T, H), o_bar.reshape(B * T, H), frames, (l, "att1")
        yield f"L{l}.lse1", "attention", lse.reshape(B * heads, T), lse_bar.reshape(B * heads, T), fh, (l, "lse1")
        # 5 h1 = h0 + (att1 proj^T + b)
        y, bar = gemm(z["att1"], sd[p + "attn.proj.weight"], r_mm)
        yb = y + sd[p + "attn.proj.bias"]
        yield f"L{l}.h1", "exact", z["h0"] + yb, bar + adds(yb, z["h0"] + yb), frames, (l, "h1")
        # 6 cross queries
        xn = rms_rows(z["h1"], sd[p + "norm2.weight"])
        ref, bar = normed_gemm(xn, ETA * xn.abs(), sd[p + "cross_attn.q_proj.weight"], r_mm, opts.mm, amb, frames)
        yield f"L{l}.qc", "norm", ref, narrowed(ref, bar), frames, (l, "qc")
        # 7 cross-attention
        k, v = (z["kv"][:, i * H:(i + 1) * H].reshape(B, S, H) for i in range(2))
        o, o_bar, lse, lse_bar = attention(z["qc"].reshape(B, T, H), k, v, heads, None, cs.s_len, r_at, opts.att, dm.get((l, 1)))
        yield f"L{l}.att2", "attention", o.reshape(B * T, H), o_bar.reshape(B * T, H), frames, (l, "att2")
        yield f"L{l}.lse2", "attention", lse.reshape(B * heads, T), lse_bar.reshape(B * heads, T), fh, (l, "lse2")
        # 8 h2 = h1 + att2 out_proj^T
        y, bar = gemm(z["att2"], sd[p + "cross_attn.out_proj.weight"], r_mm)
        yield f"L{l}.h2", "exact", z["h1"] + y, bar + adds(z["h1"] + y), frames, (l, "h2")
        # 9 SwiGLU output
        xn, d = ada_rows(z["h2"], gain(l, "norm3"), mod(l, 1))
        y, bar = normed_gemm(xn, d, sd[p + "ffn.net.0.weight"], r_mm, opts.mm, amb, frames)
        yb = y + sd[p + "ffn.net.0.bias"]
        ref, bar = swiglu(yb, bar + adds(yb), dm.get((l, 2)))
        yield f"L{l}.act", "norm+function", ref, narrowed(ref, bar), frames, (l, "act")
        # 10 the next layer's h0 (or hL) = h2 + mask o (act down^T + b)
        y, bar = gemm(z["act"], sd[p + "ffn.net.3.weight"], r_mm)
        yb = y + sd[p + "ffn.net.3.bias"]
        bar = bar + adds(yb)
        if (l, 3) in dm:
            yb, bar = yb * dm[l, 3], bar * dm[l, 3] + adds(yb * dm[l, 3])
        where = (l + 1, "h0") if l + 1 < L else (None, "hl")
        yield (f"L{l + 1}.h0" if l + 1 < L else "hl"), "exact", z["h2"] + yb, bar + adds(z["h2"] + yb), frames, where
    # 11 eps: rows past T_b are exactly 0
    xn, d = layer_rows(tp["hl"], sd["final_norm.weight"], sd["final_norm.bias"])
    y, bar = normed_gemm(xn, d, sd["out_proj.weight"], r_mm, opts.mm, amb, frames)
    yb = y + sd["out_proj.bias"]
    dead = ~frames[:, None]
    yield "eps", "norm", torch.where(dead, torch.zeros_like(yb), yb), torch.where(dead, torch.zeros_like(yb), bar + adds(yb)), None, (None, "eps")


def _slot(tp, where):
    l, which = where
    return tp if l is None else tp["layers"][l], which


def empty_tape(cs, tcond):
    return dict(tcond=tcond, layers=[{} for _ in range(cs.cfg.layers)])


def tcond64(cs):
    return O.time_condition(weights(cs), cs.inp["t"], cs.inp["si"])


def chain(cs, opts=OPTION_SETS[0], drop=None, amb=None):
    """The tape of references, each stage fed by the references before it: with no rounding, the fp64 oracle's forward."""
    tp = empty_tape(cs, tcond64(cs))
    for name, _, ref, bar, live, where in stages(cs, opts, tp, drop, amb):
        d, k = _slot(tp, where)
        d[k] = ref / LN2 if k in ("lse1", "lse2") else ref  # (the tape's log-sum-exps are in the exp2 domain)
    return tp


Result = collections.namedtuple("Result", "ratio worst_err worst_bar unwritten cls")


def audit(cs, opts, tp, drop=None, amb=None):
    """{stage: Result} of a filled tape: per stage the worst error / bar over the live elements and how many of them are not finite."""
    out = {}
    for name, cls, ref, bar, live, where in stages(cs, opts, tp, drop, amb):
        d, k = _slot(tp, where)
        got = d[k] * LN2 if k in ("lse1", "lse2") else d[k]
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        if live is not None:
            got, ref, bar = got[live], ref[live], bar[live]
        fin = torch.isfinite(got)
        assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(bar).all()) and bool((bar >= 0).all()), name
        err = torch.where(fin, (got - ref).abs(), torch.zeros_like(ref))
        ratio = (err / bar.clamp_min(1e-300)).masked_fill(err == 0, 0.0)
        i = int(ratio.argmax())
        out[name] = Result(float(ratio.reshape(-1)[i]), float(err.reshape(-1)[i]), float(bar.reshape(-1)[i]), int((~fin).sum()), cls)
    return out


def report(res, what):
    """Prints every stage's worst ratio; returns {class: worst ratio}."""
    by = {}
    for name, r in res.items():
        print(f"{what} {name:8s} {r.cls:14s} worst error / bar {r.ratio:8.3f}  (error {r.worst_err:.3e}, bar {r.worst_bar:.3e})")
        by[r.cls] = max(by.get(r.cls, 0.0), r.ratio)
    print(f"{what}: " + "  ".join(f"{c} {v:.3f}" for c, v in sorted(by.items())))
    return by


def check(res, what):
    by = report(res, what)
    bad = {k: v for k, v in res.items() if v.unwritten or not v.ratio <= 1.0}
    assert not bad, f"{what}: {bad}"
    return by


# ------------------------------------------------------------------------------------------------------------ the oracle's own error
def measure_allowances(names):
    """(eta, c_lse, c_fn) BEFORE the margin: the fp32 CPU oracle's worst error against fp64, each on the fp32 operands that the fp64
    chain of the cases produces.  eta: norm rows relative to their summands; c_lse: log-sum-exp of fp32 scores, in u max(1, |LSE|);
    c_fn: g sigmoid(g), in u |g sigmoid(g)|."""
    eta = c_lse = c_fn = 0.0

    def worst(v):  # (rows past a ragged batch's lengths are not operands of anything: not finite here)
        v = v[torch.isfinite(v)]
        return float(v.max()) if v.numel() else 0.0

    for name in names:
        cs = case(name)
        sd, tp = weights(cs), chain(cs)
        cfg, B, T, S = cs.cfg, cs.B, cs.T, cs.S
        H, heads = cfg.hidden, cfg.heads
        adaln = "layers.0.norm1.proj.weight" in sd
        cond = tp["cond"].reshape(B, cfg.layers, 2, 2 * H)

        def norm_err(x, w, m):
            x32 = x.to(F32)
            m32 = None if m is None else m.to(F32)
            y32 = O.rms_norm(x32, w.to(F32))
            if m32 is not None:
                y32 = y32 * m32[:, :H] + m32[:, H:]
            y64, d = ada_rows(x32.to(F64), w.to(F32).to(F64), None if m32 is None else m32.to(F64))
            return worst((y32.to(F64) - y64).abs() / (d / ETA).clamp_min(1e-300))

        for l in range(cfg.layers):
            z, p = tp["layers"][l], f"layers.{l}."
            for h, nm, which in ((z["h0"], "norm1", 0), (z["h2"], "norm3", 1)):
                w = sd[p + nm + ".norm.weight"] if adaln else sd[p + nm + ".weight"]
                eta = max(eta, norm_err(h, w, cond[:, l, which].repeat_interleave(T, 0) if adaln else None))
            eta = max(eta, norm_err(z["h1"], sd[p + "norm2.weight"], None), norm_err(z["crp"], sd[p + "cross_attn.kv_norm.weight"], None))
            for q, k, Tk, window, k_len in ((z["qkv"][:, :H], z["qkv"][:, H:2 * H], T, cfg.attn_window_size, cs.t_len),
                                            (z["qc"], z["kv"][:, :H], S, None, cs.s_len)):
                qh, kh = O.split_heads(q.reshape(B, T, H), heads), O.split_heads(k.reshape(B, Tk, H), heads)
                s32 = ((qh @ kh.transpose(-1, -2)) / math.sqrt(H // heads)).masked_fill(~key_mask(T, Tk, window, k_len, B), float("-inf")).to(F32)
                l64 = torch.logsumexp(s32.to(F64), dim=-1)
                c_lse = max(c_lse, worst((torch.logsumexp(s32, dim=-1).to(F64) - l64).abs() / (u * l64.abs().clamp_min(1.0))))
            xn, _ = ada_rows(z["h2"], sd[p + "norm3.norm.weight"] if adaln else sd[p + "norm3.weight"],
                             cond[:, l, 1].repeat_interleave(T, 0) if adaln else None)
            g32 = (xn @ sd[p + "ffn.net.0.weight"].T + sd[p + "ffn.net.0.bias"])[:, cfg.ffn_mult * H:].to(F32)
            s64 = g32.to(F64) * torch.sigmoid(g32.to(F64))
            c_fn = max(c_fn, worst(((g32 * torch.sigmoid(g32)).to(F64) - s64).abs() / (u * s64.abs()).clamp_min(1e-300)))
        x32 = tp["hl"].to(F32)
        y32 = O.layer_norm(x32, sd["final_norm.weight"].to(F32), sd["final_norm.bias"].to(F32))
        y64, d = layer_rows(x32.to(F64), sd["final_norm.weight"], sd["final_norm.bias"])
        eta = max(eta, worst((y32.to(F64) - y64).abs() / (d / ETA).clamp_min(1e-300)))
    return eta, c_lse, c_fn


# ------------------------------------------------------------------------------------------------------------ an fp32 emulation
# One draw of what the contract allows, in fp32 torch: every GEMM consumes K in chunks of 32, the attention is an online softmax in
# 32-key steps with P rounded to bf16 against the running maximum.  It shows that the bars can be met; its mutants, each a fault of the
# kind a kernel can have, show that they are not vacuous.  mutant: None or one of MUTANTS (name -> the stage whose bar must catch it).
MUTANTS = {
    "last_key": "L0.att1",      # the last in-band key of every query dropped
    "window": "L0.att1",        # the band one key too wide
    "key_at_len": "L0.att1",    # a ragged batch: the key at index T_b read
    "k_term_exact": "L0.crp",   # the k-term K - 1 dropped (an exact-class GEMM)
    "k_term_norm": "L0.qkv",    # ... (a norm-class GEMM)
    "unrounded_mm": "L0.qkv",   # operands left unrounded with the option on
    "unrounded_att": "L0.lse1",  # (the output's own bar carries the 2^-8 of P; the log-sum-exp's does not)
    "swap": "L0.qkv",           # the scale and shift halves swapped
    "bias": "L0.h1",            # the bias omitted
    "snapshot": "L0.h2",        # the residual taken from the wrong snapshot (h0 for h1)
    "drop_l": "L0.lse1",        # the dropout multiplier applied to l as well
}


def bf16_32(v):
    return v.to(torch.bfloat16).to(F32)


def emulate(cs, opts, drop=None, mutant=None):
    cfg, B, T, S, inp = cs.cfg, cs.B, cs.T, cs.S, cs.inp
    sd = O.cast_sd(cs.sd, F32)
    H, heads, L = cfg.hidden, cfg.heads, cfg.layers
    r_mm, r_at = (bf16_32 if opts.mm else ident), (bf16_32 if opts.att else ident)
    dm = {k: v.to(F32) for k, v in (drop or {}).items()}
    adaln = "layers.0.norm1.proj.weight" in sd

    def mm(a, w, drop_k=False, rnd=None):
        a, w = (rnd or r_mm)(a), (rnd or r_mm)(w)
        K = a.shape[-1] - (1 if drop_k else 0)
        acc = torch.zeros(a.shape[0], w.shape[0], dtype=F32)
        for k0 in range(0, K, 32):
            acc = acc + a[:, k0:min(K, k0 + 32)] @ w[:, k0:min(K, k0 + 32)].T
        return acc

    def attn(q, k, v, window, k_len, mult, first):
        Tk, d = k.shape[1], H // heads
        rnd = ident if (first and mutant == "unrounded_att") else r_at
        qh, kh, vh = (O.split_heads(rnd(z), heads) for z in (q, live_keys(k, k_len), live_keys(v, k_len)))
        if first and mutant == "window":
            window = window + 1
        kl = k_len
        if first and mutant == "key_at_len":
            kl = (k_len + 1).clamp(max=Tk)
            kh, vh = O.split_heads(rnd(k), heads), O.split_heads(rnd(v), heads)
        ok = key_mask(T, Tk, window, kl, B).expand(B, heads, T, Tk).clone()
        if first and mutant == "last_key":
            last = (ok.long() * (torch.arange(Tk) + 1)).amax(dim=-1, keepdim=True) - 1
            ok.scatter_(-1, last, False)
        scale = torch.tensor(1.4426950408889634 / math.sqrt(d), dtype=F32)
        m = torch.full((B, heads, T), -1e30, dtype=F32)
        l, acc = torch.zeros(B, heads, T, dtype=F32), torch.zeros(B, heads, T, d, dtype=F32)
        for j0 in range(0, Tk, 32):
            j1 = min(Tk, j0 + 32)
            s = ((qh @ kh[:, :, j0:j1].transpose(-1, -2)) * scale).masked_fill(~ok[..., j0:j1], float("-inf"))
            mn = torch.maximum(m, s.amax(dim=-1))
            alpha = torch.exp2(m - mn)
            p = torch.exp2(s - mn[..., None])
            pd = p if mult is None else p * mult[..., j0:j1]
            l = l * alpha + (pd if (first and mutant == "drop_l") else p).sum(dim=-1)
            acc = acc * alpha[..., None] + rnd(pd) @ vh[:, :, j0:j1]
            m = mn
        return O.merge_heads(acc / l[..., None]).reshape(B * T, H), (m + torch.log2(l)).reshape(B * heads, T)

    def ada(x, w, m):
        y = O.rms_norm(x, w)
        if m is None:
            return y
        a, b = (m[:, H:], m[:, :H]) if mutant == "swap" else (m[:, :H], m[:, H:])
        return y * a + b

    def store(v):
        return bf16_32(v) if opts.tape else v

    tp = dict(tcond=O.time_condition(sd, inp["t"], inp["si"]), layers=[{} for _ in range(L)])
    cpe = sd["context_pos_emb.pe"][:S].repeat(B, 1)
    if inp["f"] is not None:
        tp["ctx"] = mm(torch.nan_to_num(inp["f"]).reshape(B * S, -1), sd["sem_proj.weight"]) + sd["sem_proj.bias"] + cpe
    else:
        tp["ctx"] = sd["token_emb.weight"][inp["sem"].reshape(-1)] + cpe
    rows = []
    for l in range(L):
        for nm in ("norm1.", "norm3."):
            if adaln:
                y = mm(tp["tcond"], sd[f"layers.{l}.{nm}proj.weight"]) + sd[f"layers.{l}.{nm}proj.bias"]
            else:
                y = torch.zeros(B, 2 * H, dtype=F32)
            rows.append(torch.cat([1.0 + y[:, :H], y[:, H:]], 1))
    tp["cond"] = torch.stack(rows, 1).reshape(B * L * 2, 2 * H)
    cond = tp["cond"].reshape(B, L, 2, 2 * H)
    for l in range(L):
        z, p = tp["layers"][l], f"layers.{l}.cross_attn."
        z["crp"] = mm(tp["ctx"], sd[p + "kv_down_proj.weight"], drop_k=(l == 0 and mutant == "k_term_exact"))
        z["kv"] = store(mm(O.rms_norm(z["crp"], sd[p + "kv_norm.weight"]), sd[p + "kv_up_proj.weight"]))
    h = mm(torch.nan_to_num(inp["x"]).reshape(B * T, -1), sd["in_proj.weight"]) + sd["in_proj.bias"] + sd["pos_emb.pe"][:T].repeat(B, 1)
    for l in range(L):
        z, p, first = tp["layers"][l], f"layers.{l}.", l == 0
        g1, g3 = ((sd[p + "norm1.norm.weight"], sd[p + "norm3.norm.weight"]) if adaln else (sd[p + "norm1.weight"], sd[p + "norm3.weight"]))
        z["h0"] = h
        xn = ada(h, g1, cond[:, l, 0].repeat_interleave(T, 0) if adaln else None)
        z["qkv"] = store(mm(xn, sd[p + "attn.qkv.weight"], drop_k=(first and mutant == "k_term_norm"),
                            rnd=ident if (first and mutant == "unrounded_mm") else None))
        q, k, v = (z["qkv"][:, i * H:(i + 1) * H].reshape(B, T, H) for i in range(3))
        z["att1"], z["lse1"] = attn(q, k, v, cfg.attn_window_size, cs.t_len, dm.get((l, 0)), first)
        y = mm(z["att1"], sd[p + "attn.proj.weight"])
        h = h + (y if (first and mutant == "bias") else y + sd[p + "attn.proj.bias"])
        z["h1"] = h
        z["qc"] = store(mm(O.rms_norm(h, sd[p + "norm2.weight"]), sd[p + "cross_attn.q_proj.weight"]))
        k, v = (z["kv"][:, i * H:(i + 1) * H].reshape(B, S, H) for i in range(2))
        z["att2"], z["lse2"] = attn(z["qc"].reshape(B, T, H), k, v, None, cs.s_len, dm.get((l, 1)), False)
        h = (z["h0"] if (first and mutant == "snapshot") else h) + mm(z["att2"], sd[p + "cross_attn.out_proj.weight"])
        z["h2"] = h
        uu = mm(ada(h, g3, cond[:, l, 1].repeat_interleave(T, 0) if adaln else None), sd[p + "ffn.net.0.weight"]) + sd[p + "ffn.net.0.bias"]
        half = uu.shape[-1] // 2
        act = uu[:, :half] * (uu[:, half:] * torch.sigmoid(uu[:, half:]))
        z["act"] = store(act * dm[l, 2] if (l, 2) in dm else act)
        y = mm(z["act"], sd[p + "ffn.net.3.weight"]) + sd[p + "ffn.net.3.bias"]
        h = h + (y * dm[l, 3] if (l, 3) in dm else y)
    tp["hl"] = h
    eps = mm(O.layer_norm(h, sd["final_norm.weight"], sd["final_norm.bias"]), sd["out_proj.weight"]) + sd["out_proj.bias"]
    tp["eps"] = torch.where(row_mask(cs.t_len, B, T)[:, None], eps, torch.zeros_like(eps))
    return to64(tp)


def to64(tp):
    return {k: ([to64(z) for z in v] if k == "layers" else v.to(F64)) for k, v in tp.items()}
