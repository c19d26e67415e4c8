"""Shared by tests/test_bwd_audit_host.py and tests/test_bwd_audit_gpu.py: the stage-by-stage audit of the generic training backward
(DESIGN.md section 33).  edtts_decoder_backward_until stops the backward after any site of its launch list; with the scratch filled
with 0xFF before every call, what site k wrote is compared element by element with an fp64 evaluation of the operands that site k
read -- the state the call stopped at site k - 1 left, the tape, the inputs and the state dict -- under the rounding contract of
include/edtts.h.  tests/tape_audit_util.py (section 29, the forward) supplies the cases, the option sets and the small pieces.

A "state" is a dict of fp64 CPU tensors: the scratch members by their SCRATCH_REGIONS name (2-D, rows x pitch), gradient
destinations as "g:<state-dict name>", "d_x" and "d_sem".  Every site is written once (`_site`), against a backend: `Ref` evaluates
in fp64 and returns a bar with every value, `Emu` is one fp32 draw of what the contract allows (K in chunks, dW in dw_slab_rows
slabs added in slab order, bias sums in 256-row slabs, norm columns in 64-row chunks, attention sums in 16-row steps) and carries the
mutants.

Bars (u = 2^-24; rnd = bf16 round-to-nearest-even where the contract rounds, else the identity):
  contraction  K u sum|a||b| for dX, dW, bias sums, norm column sums, delta, scatters -- K the full contraction length (for sums over
               rows: the live rows, however they are cut into slabs and chunks); 2 u |r| per accumulate or epilogue operation
  recompute    the norm rows written to xn / crn: section 29's ETA relative to the summands; their consumers read them exactly
  norm_bwd     dx: ETA_B x rs (|gn| + |xhat| mean(|gn||xhat|)) (LayerNorm: + mean|gx|); column sums: the contraction term plus
               ETA |xhat| per summand for the kernel's own rstd (and mean)
  attention    S = rnd(q) rnd(k)^T / sqrt(d) with (d + 2) u sum|q||k| / sqrt(d); P = exp(S - LSE) with the TAPE's log-sum-exp, relative
               error e_S + (C_LSE + 1) u max(1, |S - LSE|); dP = rnd(dO) rnd(v)^T; dS = P (D dP - delta) with the site's own delta;
               dQ, dK, dV contract rnd(dS), rnd(P D): their errors enter as e |other operand|, under bf16 attention plus 2^-8 per
               summand (ATT_BRACKET below: the bracket of section 29 would need fewer undecided elements than the reference has)
  function     C_SW for the gate derivative of SwiGLU (C_FN, section 29's, for g sigmoid(g)), C_GELU / C_GELUD for the time MLP, C_TRIG
               for its sin / cos
The function allowances are train_util.MARGIN times the fp32 CPU evaluation's worst error against fp64 on the audit cases, rounded up
to a power of two (measure_allowances; the host test asserts that they still are).  Nothing is fitted to what the kernels give."""
import collections
import math

import torch

import tape_audit_util as TA
from edge_diffusion_tts_amd import native
from oracle import edtts_oracle as O
from tape_audit_util import F32, F64, LN2, bf16, ident, u
from train_util import MARGIN

ETA_B = 2.0 ** -19    # norm_bwd's dx, relative to rs (|gn| + |xhat| mean(|gn||xhat|))
C_SW = 16.0           # sigmoid(g) (1 + g (1 - sigmoid(g))), in units of u sigmoid(g) (1 + |g| (1 - sigmoid(g)))
C_GELU = 8.0          # GELU(x), in units of u |x|
C_GELUD = 16.0        # GELU'(x), in units of u (Phi(x) + |x| phi(x))
C_TRIG = 4.0          # sin / cos of an fp32 argument, in units of u
# rnd(dS) and rnd(P D) under bf16 attention: the bracket of section 29 (True) or a 2^-8 relative term per summand (False).  The
# bracket needs all but AMBIGUOUS_MAX of every stage's operand decided on every case; the worst-case error bounds of dS leave up to
# 1.9 % undecided (G1's cross-attention), so the relative term stands (the host test measures the share and asserts this choice).
ATT_BRACKET = False
ALLOWANCES = ("ETA_B", "C_SW", "C_GELU", "C_GELUD", "C_TRIG")
D_EPS_SEED = 33

HEAD, LAYER = ("out", "fnorm"), native.BWD_LAYER_SITES
Out = collections.namedtuple("Out", "ref bar live dead")  # live: row mask or None; dead: "zero" = rows outside `live` are exactly 0


def d_eps_of(cs):
    """The upstream gradient of every run: seeded randn of eps's shape (a loss gradient would be about 1e-4 small and uniform)."""
    return torch.randn(cs.B, cs.T, cs.cfg.n_mels, generator=torch.Generator().manual_seed(D_EPS_SEED + cs.B * 1000 + cs.T))


class Ctx:
    """What does not change during a backward: the case, the options, the tape (tape_audit_util's dict, fp64), d_eps, the dropout
    multipliers {(layer, site): tensor} and the row masks."""

    def __init__(self, cs, opts, tape, drop=None, d_eps=None):
        self.cs, self.opts, self.tp, self.dm = cs, opts, tape, drop or {}
        self.sd = TA.weights(cs)
        cfg = cs.cfg
        self.B, self.T, self.S, self.H, self.heads, self.L = cs.B, cs.T, cs.S, cfg.hidden, cfg.heads, cfg.layers
        self.adaln = "layers.0.norm1.proj.weight" in self.sd
        self.feats, self.with_step = cs.inp["f"] is not None, cs.inp["si"] is not None
        self.frames, self.toks = TA.row_mask(cs.t_len, cs.B, cs.T), TA.row_mask(cs.s_len, cs.B, cs.S)
        self.d_eps = (d_eps_of(cs) if d_eps is None else d_eps).to(F64).reshape(cs.B * cs.T, -1)
        self.x = cs.inp["x"].to(F64).reshape(cs.B * cs.T, -1)
        self.f = None if not self.feats else cs.inp["f"].to(F64).reshape(cs.B * cs.S, -1)
        self.cond = tape["cond"].reshape(cs.B, self.L, 2, 2 * self.H)

    def sites(self):
        """[(layer, site name)] in launch order, of the sites this configuration has."""
        out = [(0, s) for s in HEAD]
        for l in range(self.L - 1, -1, -1):
            out += [(l, s) for s in LAYER if s != "dropdown" or self.dm]
        out += [(0, "inp"), (0, "sem")]
        if self.adaln:
            out += [(0, "ada")] + ([(0, "step")] if self.with_step else []) + [(0, "time")]
        return out

    def gain(self, l, nm):
        return self.sd[f"layers.{l}.{nm}.norm.weight" if self.adaln else f"layers.{l}.{nm}.weight"]

    def gain_name(self, l, nm):
        return f"g:layers.{l}.{nm}.norm.weight" if self.adaln else f"g:layers.{l}.{nm}.weight"

    def mod(self, l, which):
        """[B, 2H]: (1 + scale | shift) of one AdaLN norm, as the tape holds it (plain RMSNorm blocks: ones | zeros)."""
        return self.cond[:, l, which]


def _rows(v, live):
    """Rows outside `live` are never loaded: zero (the padding may hold NaN)."""
    return v if live is None else torch.where(live[:, None], v, torch.zeros_like(v))


def _all(n):
    return torch.ones(n, dtype=torch.bool)


# ------------------------------------------------------------------------------------------------------------ the fp64 backend
class Ref:
    """Every method returns (value, bar)."""

    def __init__(self, cx, amb=None, measure=None):
        self.cx, self.amb, self.measure = cx, amb, measure
        self.r_mm, self.r_at = (bf16 if cx.opts.mm else ident), (bf16 if cx.opts.att else ident)

    def _worst(self, key, err, scale):
        if self.measure is not None:
            r = (err / scale.clamp_min(1e-300))[torch.isfinite(err) & (scale > 0)]
            if r.numel():
                self.measure[key] = max(self.measure.get(key, 0.0), float(r.max()))

    # ---- contractions
    def dx(self, key, dY, W, live, pre=None):
        a, w = self.r_mm(_rows(dY, live)), self.r_mm(W)
        ref, bar = a @ w, (a.shape[1] * u) * (a.abs() @ w.abs())
        if pre is not None:
            ref = _rows(pre, live) + ref
            bar = bar + TA.adds(ref)
        return ref, bar

    def dw(self, key, dY, X, live):
        a, x = self.r_mm(dY[live]), self.r_mm(X[live])
        return a.T @ x, (a.shape[0] * u) * (a.abs().T @ x.abs())

    def colsum(self, key, Y, live):
        y = Y[live]
        return y.sum(0), (y.shape[0] * u) * y.abs().sum(0)

    def linear(self, key, x, W, b):
        y, bar = TA.gemm(x, W, self.r_mm)
        return y + b, bar + TA.adds(y + b)

    def mul(self, key, x, mult):
        return x * mult, TA.adds(x * mult)

    def scatter(self, key, idx, src, n_rows, live):
        hit = (idx[None, :] == torch.arange(n_rows)[:, None]) & live[None, :]
        s = torch.nan_to_num(src)
        return hit.to(F64) @ s, (hit.sum(1, keepdim=True).to(F64) * u) * (hit.to(F64) @ s.abs())

    # ---- norms
    def rms_rows(self, key, x, w, mod_rows):
        return TA.ada_rows(x, w, mod_rows)

    def layer_rows(self, key, x, w, b):
        return TA.layer_rows(x, w, b)

    def norm_bwd(self, key, mode, x, dy, w, mod, pre, live, B):
        """dx (+ pre), gain gradient, and LayerNorm: bias gradient / RMSNorm with mod [B, 2H]: dmod [B, 2H] (dscale | dshift).
        Returns {name: (ref, bar)} for "dx", "gain", "bias" / "dmod"."""
        n, W = x.shape[0] // B, x.shape[1]
        x, dy = _rows(x, live), _rows(dy, live)
        sc = torch.ones_like(x) if mod is None else mod[:, :W].repeat_interleave(n, 0)
        if mode == "layer":
            mu = x.mean(-1, keepdim=True)
            rs = torch.rsqrt((x - mu).pow(2).mean(-1, keepdim=True) + 1e-5)
            xh, xh_err = (x - mu) * rs, TA.ETA * (x.abs() + mu.abs()) * rs
            gn = dy * w
            v = rs * (gn - gn.mean(-1, keepdim=True) - xh * (gn * xh).mean(-1, keepdim=True))
            mag = rs * (gn.abs() + gn.abs().mean(-1, keepdim=True) + xh.abs() * (gn.abs() * xh.abs()).mean(-1, keepdim=True))
        else:
            rs = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-6)
            xh, xh_err = x * rs, TA.ETA * (x * rs).abs()
            gn = dy * w * sc
            v = rs * (gn - xh * (gn * xh).mean(-1, keepdim=True))
            mag = rs * (gn.abs() + xh.abs() * (gn.abs() * xh.abs()).mean(-1, keepdim=True))
        if self.measure is not None:
            x32, d32, w32, s32 = x.to(F32), dy.to(F32), w.to(F32), sc.to(F32)
            x64, d64 = x32.to(F64), d32.to(F64)
            if mode == "layer":
                def f(xx, dd, ww, ss):
                    m = xx.mean(-1, keepdim=True)
                    r = torch.rsqrt((xx - m).pow(2).mean(-1, keepdim=True) + 1e-5)
                    g, h = dd * ww, (xx - m) * r
                    return r * (g - g.mean(-1, keepdim=True) - h * (g * h).mean(-1, keepdim=True))
            else:
                def f(xx, dd, ww, ss):
                    r = torch.rsqrt(xx.pow(2).mean(-1, keepdim=True) + 1e-6)
                    g, h = dd * ww * ss, xx * r
                    return r * (g - h * (g * h).mean(-1, keepdim=True))
            self._worst("ETA_B", (f(x32, d32, w32, s32).to(F64) - f(x64, d64, w32.to(F64), s32.to(F64))).abs()[live], mag[live])
        dx, bar = v, ETA_B * mag
        if pre is not None:
            dx = _rows(pre, live) + v
            bar = bar + TA.adds(dx)
        out = {"dx": (dx, bar)}

        def colsum(terms, err, rows):  # a sum over live rows of exact-operand products whose xhat the kernel formed itself
            t, e = terms[rows], err[rows]
            return t.sum(0), ((t.shape[0] + 4) * u) * t.abs().sum(0) + e.sum(0)

        out["gain"] = colsum(dy * sc * xh, (dy * sc).abs() * xh_err, live)
        if mode == "layer":
            out["bias"] = colsum(dy, torch.zeros_like(dy), live)
        elif mod is not None:
            parts = []
            for b in range(B):
                rows = live & (torch.arange(x.shape[0]) // n == b)
                ds_, de_ = colsum(dy * (xh * w), dy.abs() * xh_err * w.abs(), rows)
                sh_, se_ = colsum(dy, torch.zeros_like(dy), rows)
                parts.append((torch.cat([ds_, sh_]), torch.cat([de_, se_])))
            out["dmod"] = (torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]))
        return out

    # ---- functions
    def swiglu_bwd(self, key, big, da, mult):
        FH = da.shape[1]
        v, g = big[:, :FH], big[:, FH:]
        d, e = (da, 0.0) if mult is None else (da * mult, 2 * u)
        sg = torch.sigmoid(g)
        fac, fmag = sg * (1 + g * (1 - sg)), sg * (1 + g.abs() * (1 - sg))
        if self.measure is not None:
            g32 = g.to(F32)
            s32, s64 = torch.sigmoid(g32), torch.sigmoid(g32.to(F64))
            f32_, f64_ = s32 * (1 + g32 * (1 - s32)), s64 * (1 + g32.to(F64) * (1 - s64))
            self._worst("C_SW", (f32_.to(F64) - f64_).abs(), u * s64 * (1 + g32.to(F64).abs() * (1 - s64)))
        gv, gg = d * (g * sg), d * v * fac
        bar_v = ((TA.C_FN + 2) * u + e) * gv.abs()
        bar_g = ((C_SW + 4) * u + e) * (d * v).abs() * fmag
        return torch.cat([gv, gg], 1), torch.cat([bar_v, bar_g], 1)

    def time_emb(self, key, t, freqs):
        arg = t.to(F64)[:, None] * freqs.to(F64)[None, :]
        if self.measure is not None:
            a32 = t.float()[:, None] * freqs[None, :]
            e32, e64 = torch.cat([torch.sin(a32), torch.cos(a32)], 1), torch.cat([torch.sin(a32.to(F64)), torch.cos(a32.to(F64))], 1)
            self._worst("C_TRIG", (e32.to(F64) - e64).abs(), torch.full_like(e64, u))
        e = torch.cat([torch.sin(arg), torch.cos(arg)], 1)
        return e, (u * arg.abs() + C_TRIG * u).repeat(1, 2)  # (the fp32 product t f is rounded before the sin)

    def gelu(self, key, a1):
        if self.measure is not None:
            x32 = a1.to(F32)
            self._worst("C_GELU", (O.gelu_erf(x32).to(F64) - O.gelu_erf(x32.to(F64))).abs(), u * x32.to(F64).abs())
        return O.gelu_erf(a1), (C_GELU * u) * a1.abs()

    def gelu_grad(self, key, du, a1):
        def parts(x):
            return 0.5 * (1 + torch.erf(x / math.sqrt(2.0))), x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)
        cdf, xpdf = parts(a1)
        if self.measure is not None:
            x32 = a1.to(F32)
            c32, p32 = parts(x32)
            c64, p64 = parts(x32.to(F64))
            self._worst("C_GELUD", ((c32 + p32).to(F64) - (c64 + p64)).abs(), u * (c64 + p64.abs()))
        r = du * (cdf + xpdf)
        return r, ((C_GELUD + 2) * u) * du.abs() * (cdf + xpdf.abs())

    # ---- attention
    def attn_bwd(self, key, q, k, v, o, dO, lse2, window, q_len, k_len, mult, delta_used=None):
        """q, o, dO [B, T, H]; k, v [B, Tk, H]; lse2 [B, heads, T] in the exp2 domain.  Returns {"delta", "dq", "dk", "dv"}:
        delta [B heads, T], dq [B T, H], dk / dv [B Tk, H]; delta_used: the site's own delta (None: the reference's)."""
        cx, r = self.cx, self.r_at
        B, T, H = q.shape
        Tk, heads, d = k.shape[1], cx.heads, H // cx.heads
        sq = 1.0 / math.sqrt(d)
        qlive = torch.ones(B, T, dtype=torch.bool) if q_len is None else torch.arange(T)[None, :] < q_len[:, None]
        ok = TA.key_mask(T, Tk, window, k_len, B).expand(B, heads, T, Tk) & qlive[:, None, :, None]
        q, o, dO = (TA.live_keys(z, q_len) for z in (q, o, dO))
        k, v = TA.live_keys(k, k_len), TA.live_keys(v, k_len)
        oh, dOh = O.split_heads(o, heads), O.split_heads(dO, heads)
        delta = (oh * dOh).sum(-1)
        out = {"delta": (delta.reshape(B * heads, T), ((d * u) * (oh * dOh).abs().sum(-1)).reshape(B * heads, T))}
        dl = delta if delta_used is None else delta_used.reshape(B, heads, T)
        qh, kh, vh, rdO = (O.split_heads(r(z), heads) for z in (q, k, v, dO))
        s = (qh @ kh.transpose(-1, -2)) * sq
        e_s = ((d + 2) * u * sq) * (qh.abs() @ kh.abs().transpose(-1, -2))
        a = torch.where(ok, s - (lse2 * LN2)[..., None], torch.zeros_like(s))
        p = torch.where(ok, torch.exp(a), torch.zeros_like(s))
        relp = e_s + ((TA.C_LSE + 1) * u) * a.abs().clamp_min(1.0)
        dp, e_dp = rdO @ vh.transpose(-1, -2), (d * u) * (rdO.abs() @ vh.abs().transpose(-1, -2))
        if mult is not None:
            dp, e_dp = dp * mult, e_dp * mult + TA.adds(dp * mult)
        pd = p if mult is None else p * mult
        e_pd = (relp + (2 * u if mult is not None else 0.0)) * pd
        ds = p * (dp - dl[..., None])
        e_ds = p * (e_dp + u * (dp - dl[..., None]).abs()) + (relp + 2 * u) * ds.abs()
        n_q, n_k = ok.sum(-1, keepdim=True).to(F64), ok.sum(-2).to(F64)[..., None]  # live in-band keys per query / queries per key

        def contract(x, e_x, other, n, scale, what, band):  # rnd(x) @ other * scale; band: the elements of x that are summed
            if cx.opts.att and self.amb is not None:  # (the share that decides ATT_BRACKET: the host test)
                self.amb.append((f"{site_id(key)}.{what}", float((r(x - e_x) != r(x + e_x))[band].double().mean())))
            if cx.opts.att and ATT_BRACKET:
                lo, hi = r(x - e_x), r(x + e_x)
                xr, extra = r(x), (hi - lo).abs() @ other.abs()
            elif cx.opts.att:
                xr = r(x)
                extra = 2.0 ** -8 * (xr.abs() @ other.abs()) + e_x @ other.abs()
            else:
                xr, extra = x, e_x @ other.abs()
            ref = (xr @ other) * scale
            return ref, (n * u * (xr.abs() @ other.abs()) + extra) * scale + 2 * u * ref.abs()

        okT = ok.transpose(-1, -2)
        dq = contract(ds, e_ds, kh, n_q, sq, "dq", ok)
        dk = contract(ds.transpose(-1, -2), e_ds.transpose(-1, -2), qh, n_k, sq, "dk", okT)
        dv = contract(pd.transpose(-1, -2), e_pd.transpose(-1, -2), rdO, n_k, 1.0, "dv", okT)
        for nm, (ref, bar), rows in (("dq", dq, T), ("dk", dk, Tk), ("dv", dv, Tk)):
            out[nm] = (O.merge_heads(ref).reshape(B * rows, H), O.merge_heads(bar).reshape(B * rows, H))
        return out


# ------------------------------------------------------------------------------------------------------------ an fp32 emulation
MUTANTS = {  # name -> (site, layer: "last" = L - 1, "first" = 0, output that must fail, what it is)
    "dkv_tile": ("self", "last", "big", "dK/dV: the furthest in-band query tile of every key tile dropped"),
    "dq_band": ("self", "last", "big", "dQ: the band one key too wide"),
    "row_at_len": ("self", "last", "big", "ragged: the key row at index T_b read"),
    "dw_last_row": ("down", "last", "g:layers.{l}.ffn.net.3.weight", "dW: the last row of the last slab dropped"),
    "dw_dead_row": ("out", "last", "g:out_proj.weight", "dW: a dead row included"),
    "bias_rounded": ("down", "last", "g:layers.{l}.ffn.net.3.bias", "the bias gradient taken from the rounded dY"),
    "delta_rounded": ("self", "last", "delta", "delta taken from rounded O / dO"),
    "drop_delta": ("self", "last", "big", "the dropout multiplier applied to the delta term as well"),
    "swiglu_swap": ("swiglu", "last", "big", "value and gate gradients swapped"),
    "ada_swap": ("n3", "last", "dmod", "dscale / dshift halves swapped"),
    "n3_scale": ("n3", "last", "dh", "the 1 + scale factor omitted in norm3's dx"),
    "dh_overwrite": ("n3", "last", "dh", "dh overwritten where it accumulates"),
    "dctx_last": ("kvd", "first", "dctx", "dctx taken from the last layer processed only"),
    "unrounded": ("down", "last", "da", "an operand left unrounded with its option on"),
}


def bf16_32(v):
    return v.to(torch.bfloat16).to(F32)


class Emu:
    """One fp32 draw of the contract; every method returns (value as fp64, None).  mutant: (name, site key) or None."""

    def __init__(self, cx, mutant=None, at=None):
        self.cx, self.mutant, self.at = cx, mutant, at
        self.r_mm, self.r_at = (bf16_32 if cx.opts.mm else ident), (bf16_32 if cx.opts.att else ident)

    def _m(self, name, key):
        return self.mutant == name and key == self.at

    @staticmethod
    def _mm(a, b, chunk=32):
        acc = torch.zeros(a.shape[:-1] + b.shape[-1:], dtype=F32)
        for k0 in range(0, a.shape[-1], chunk):
            acc = acc + a[..., k0:k0 + chunk] @ b[..., k0:k0 + chunk, :]
        return acc

    def dx(self, key, dY, W, live, pre=None):
        rnd = ident if self._m("unrounded", key) else self.r_mm
        y = self._mm(rnd(_rows(dY, live).to(F32)), rnd(W.to(F32)))
        if pre is not None:
            y = _rows(pre, live).to(F32) + y
        return y.to(F64), None

    def dw(self, key, dY, X, live):
        M = dY.shape[0]
        live = live.clone()
        if self._m("dw_last_row", key):
            live[int(live.nonzero().max())] = False
        if self._m("dw_dead_row", key):
            dead = (~live).nonzero()
            if dead.numel():
                live[int(dead.min())] = True
        a, x = self.r_mm(torch.nan_to_num(_rows(dY, live)).to(F32)), self.r_mm(torch.nan_to_num(_rows(X, live)).to(F32))
        rows, acc = native.train_dw_slab_rows(M), None
        for r0 in range(0, M, rows):
            part = self._mm(a[r0:r0 + rows].T.contiguous(), x[r0:r0 + rows], 16)
            acc = part if acc is None else acc + part
        return acc.to(F64), None

    def colsum(self, key, Y, live):
        y = _rows(Y, live).to(F32)
        if self._m("bias_rounded", key):
            y = self.r_mm(y)
        acc = None
        for r0 in range(0, y.shape[0], 256):
            sl = y[r0:r0 + 256]
            g = [sl[i::4].sum(0) for i in range(4)]
            part = ((g[0] + g[1]) + g[2]) + g[3]
            acc = part if acc is None else acc + part
        return acc.to(F64), None

    def linear(self, key, x, W, b):
        return (self._mm(self.r_mm(x.to(F32)), self.r_mm(W.to(F32)).T) + b.to(F32)).to(F64), None

    def mul(self, key, x, mult):
        return (x.to(F32) * mult.to(F32)).to(F64), None

    def scatter(self, key, idx, src, n_rows, live):
        out = torch.zeros(n_rows, src.shape[1], dtype=F32)
        s = src.to(F32)
        for p in range(idx.numel()):
            if bool(live[p]):
                out[int(idx[p])] += s[p]
        return out.to(F64), None

    def rms_rows(self, key, x, w, mod_rows):
        y = O.rms_norm(torch.nan_to_num(x).to(F32), w.to(F32))
        if mod_rows is not None:
            H = x.shape[1]
            y = y * mod_rows[:, :H].to(F32) + mod_rows[:, H:].to(F32)
        return y.to(F64), None

    def layer_rows(self, key, x, w, b):
        return O.layer_norm(torch.nan_to_num(x).to(F32), w.to(F32), b.to(F32)).to(F64), None

    def norm_bwd(self, key, mode, x, dy, w, mod, pre, live, B):
        n, W = x.shape[0] // B, x.shape[1]
        x, dy, w = _rows(x, live).to(F32), _rows(dy, live).to(F32), w.to(F32)
        sc = torch.ones_like(x) if mod is None else mod[:, :W].to(F32).repeat_interleave(n, 0)
        if self._m("n3_scale", key):
            sc = torch.ones_like(x)
        if mode == "layer":
            mu = x.sum(-1, keepdim=True) / W
            rs = torch.rsqrt((x - mu).pow(2).sum(-1, keepdim=True) / W + 1e-5)
            xh, gn = (x - mu) * rs, dy * w
            v = rs * (gn - gn.sum(-1, keepdim=True) / W - xh * ((gn * xh).sum(-1, keepdim=True) / W))
        else:
            rs = torch.rsqrt(x.pow(2).sum(-1, keepdim=True) / W + 1e-6)
            xh, gn = x * rs, dy * w * sc
            v = rs * (gn - xh * ((gn * xh).sum(-1, keepdim=True) / W))
        v = _rows(v, live)
        if pre is not None and not self._m("dh_overwrite", key):
            v = _rows(pre, live).to(F32) + v
        out = {"dx": (v.to(F64), None)}
        sc_c = torch.ones_like(x) if mod is None else mod[:, :W].to(F32).repeat_interleave(n, 0)

        def cols(terms, batches):  # 64-row chunks of each utterance's live rows, added in chunk order
            acc = None
            for b in batches:
                nb = int(live[b * n:(b + 1) * n].sum())
                for r0 in range(0, n, 64):
                    sl = terms[b * n + r0:b * n + min(r0 + 64, nb)]
                    g = [sl[i::4].sum(0) for i in range(4)]
                    part = ((g[0] + g[1]) + g[2]) + g[3]
                    acc = part if acc is None else acc + part
            return acc.to(F64)

        out["gain"] = (cols(dy * sc_c * xh, range(B)), None)
        if mode == "layer":
            out["bias"] = (cols(dy, range(B)), None)
        elif mod is not None:
            halves = [torch.stack([cols(t, [b]) for b in range(B)]) for t in (dy * (xh * w), dy)]
            if self._m("ada_swap", key):
                halves.reverse()
            out["dmod"] = (torch.cat(halves, 1), None)
        return out

    def swiglu_bwd(self, key, big, da, mult):
        FH = da.shape[1]
        v, g, d = big[:, :FH].to(F32), big[:, FH:].to(F32), da.to(F32)
        if mult is not None:
            d = d * mult.to(F32)
        sg = 1.0 / (1.0 + torch.exp(-g))
        gv, gg = d * (g * sg), d * v * (sg * (1.0 + g * (1.0 - sg)))
        if self._m("swiglu_swap", key):
            gv, gg = gg, gv
        return torch.cat([gv, gg], 1).to(F64), None

    def time_emb(self, key, t, freqs):
        a = t.float()[:, None] * freqs[None, :]
        return torch.cat([torch.sin(a), torch.cos(a)], 1).to(F64), None

    def gelu(self, key, a1):
        return O.gelu_erf(a1.to(F32)).to(F64), None

    def gelu_grad(self, key, du, a1):
        x = a1.to(F32)
        return (du.to(F32) * (0.5 * (1.0 + torch.erf(x * 0.7071067811865476)) + x * 0.3989422804014327 * torch.exp(-0.5 * x * x))).to(F64), None

    def attn_bwd(self, key, q, k, v, o, dO, lse2, window, q_len, k_len, mult, delta_used=None):
        cx = self.cx
        B, T, H = q.shape
        Tk, heads, d = k.shape[1], cx.heads, H // cx.heads
        rb = 64 if cx.opts.att else 16  # rows per block of the kernels
        r = self.r_at
        qlive = torch.ones(B, T, dtype=torch.bool) if q_len is None else torch.arange(T)[None, :] < q_len[:, None]
        kl = k_len
        if self._m("row_at_len", key) and k_len is not None:
            kl = (k_len + 1).clamp(max=Tk)
        q, o, dO, k, v = (torch.nan_to_num(z).to(F32) for z in (q, o, dO, k, v))
        q, o, dO = (TA.live_keys(z, q_len) for z in (q, o, dO))
        k, v = TA.live_keys(k, kl), TA.live_keys(v, kl)
        ok = TA.key_mask(T, Tk, window, k_len, B).expand(B, heads, T, Tk) & qlive[:, None, :, None]
        ok_q = ok
        if self._m("dq_band", key) and window is not None:
            ok_q = TA.key_mask(T, Tk, window + 1, k_len, B).expand(B, heads, T, Tk) & qlive[:, None, :, None]
        if self._m("row_at_len", key):
            ok_q = TA.key_mask(T, Tk, window, kl, B).expand(B, heads, T, Tk) & qlive[:, None, :, None]
        ok_k = ok
        if self._m("dkv_tile", key):  # key tile k0: query tiles lo, lo + 16, ... < hi; the last one is not visited
            ok_k = ok.clone()
            for k0 in range(0, Tk, rb):
                lo, hi = (0, T) if window is None else (max(k0 - window, 0), min(k0 + rb + window, T))
                for b in range(B):
                    hb = min(hi, int(q_len[b])) if q_len is not None else hi
                    if hb > lo:
                        ok_k[b, :, lo + (hb - lo - 1) // 16 * 16:hb, k0:k0 + rb] = False
        oh, dOh = O.split_heads(o, heads), O.split_heads(dO, heads)
        if self._m("delta_rounded", key):
            delta = (bf16_32(oh) * bf16_32(dOh)).sum(-1)
        else:
            delta = torch.zeros(B, heads, T, dtype=F32)
            for j in range(d):
                delta = delta + oh[..., j] * dOh[..., j]
        out = {"delta": (delta.reshape(B * heads, T).to(F64), None)}
        qh, kh, vh, rdO = (O.split_heads(r(z), heads) for z in (q, k, v, dO))
        scale = torch.tensor(1.4426950408889634 / math.sqrt(d), dtype=F32)
        sn = torch.tensor(1.0 / math.sqrt(d), dtype=F32)
        sc = self._mm(qh, kh.transpose(-1, -2).contiguous(), 4) * scale
        dp = self._mm(rdO, vh.transpose(-1, -2).contiguous(), 4)
        m32 = None if mult is None else mult.to(F32)
        if m32 is not None:
            dp = dp * m32
        ls = lse2.to(F32)[..., None]
        dlt = delta[..., None]

        def probs(mask):
            p = torch.where(mask, torch.exp2(sc - ls), torch.zeros_like(sc))
            inner = dp - dlt
            if self._m("drop_delta", key) and m32 is not None:
                inner = dp - dlt * m32
            return p, p * inner

        _, ds_q = probs(ok_q)
        p_k, ds_k = probs(ok_k)
        pd_k = p_k if m32 is None else p_k * m32
        dq = self._mm(r(ds_q), kh, 16) * sn
        dk = self._mm(r(ds_k).transpose(-1, -2).contiguous(), qh, 16) * sn
        dv = self._mm(r(pd_k).transpose(-1, -2).contiguous(), rdO, 16)
        for nm, val, rows in (("dq", dq, T), ("dk", dk, Tk), ("dv", dv, Tk)):
            out[nm] = (O.merge_heads(val).reshape(B * rows, H).to(F64), None)
        return out


# ------------------------------------------------------------------------------------------------------------ the sites
def _site(cx, key, st, A, got=None):
    """{output name: Out} of site `key` = (layer, name): what it writes, from the state `st` the site before it left.  `got`: what the
    audited run wrote at this site (operands that a site writes and then reads itself -- xn, crn, delta, the time MLP's rows -- are
    taken from there, so every reference reads exact operands); None: the backend's own values (chaining)."""
    l, name = key
    sd, tp, B, T, S, H, L = cx.sd, cx.tp, cx.B, cx.T, cx.S, cx.H, cx.L
    fr, tk = cx.frames, cx.toks
    p = f"layers.{l}."
    z = tp["layers"][l]
    out = {}

    def put(nm, val, live=None, dead=None):
        out[nm] = Out(val[0], val[1], live, dead)

    def own(nm):  # an operand this site wrote itself
        return out[nm].ref if got is None else got[nm]

    def linear_bwd(dY, X, W, live, db, dw, dx_name, pre=None):
        if db:
            put(db, A.colsum(key, dY, live))
        if dw:
            put(dw, A.dw(key, dY, X, live))
        if dx_name:
            put(dx_name, A.dx(key, dY, W, live, pre), live, None if pre is not None else "zero")

    def norm_bwd(mode, x, dy, w, mod, pre, live, nb, dx_name, gain, bias=None, dmod_at=None):
        r = A.norm_bwd(key, mode, x, dy, w, mod, pre, live, nb)
        put(dx_name, r["dx"], live, None if pre is not None else "zero")
        put(gain, r["gain"])
        if bias:
            put(bias, r["bias"])
        if dmod_at is not None:
            ref, bar = r["dmod"]
            full_r = st["dmod"].reshape(B, L, 2, 2 * H).clone() if "dmod" in st else torch.full((B, L, 2, 2 * H), float("nan"), dtype=F64)
            full_r[:, dmod_at[0], dmod_at[1]] = ref
            mask = torch.zeros(B, L, 2, 2 * H, dtype=torch.bool)
            mask[:, dmod_at[0], dmod_at[1]] = True
            full_b = torch.zeros(B, L, 2, 2 * H, dtype=F64)
            if bar is not None:
                full_b[:, dmod_at[0], dmod_at[1]] = bar
            out["dmod"] = Out(full_r.reshape(B * L * 2, 2 * H), None if bar is None else full_b.reshape(B * L * 2, 2 * H),
                              mask.reshape(B * L * 2, 2 * H), None)

    def attn(q, k, v, o, dO, lse, window, q_len, k_len, mult):
        r = A.attn_bwd(key, q, k, v, o, dO, lse, window, q_len, k_len, mult)
        put("delta", r["delta"], None, None)
        if got is not None:
            r = A.attn_bwd(key, q, k, v, o, dO, lse, window, q_len, k_len, mult, delta_used=got["delta"])
        return r

    if name == "out":
        put("dctx", (torch.zeros(B * S, H, dtype=F64), torch.zeros(B * S, H, dtype=F64) if isinstance(A, Ref) else None))
        put("g:out_proj.bias", A.colsum(key, cx.d_eps, fr))
        put("xn", A.layer_rows(key, tp["hl"], sd["final_norm.weight"], sd["final_norm.bias"]), fr)
        linear_bwd(cx.d_eps, own("xn"), sd["out_proj.weight"], fr, None, "g:out_proj.weight", "ga")
    elif name == "fnorm":
        norm_bwd("layer", tp["hl"], st["ga"], sd["final_norm.weight"], None, None, fr, B, "dh", "g:final_norm.weight", "g:final_norm.bias")
    elif name == "dropdown":
        put("gq", A.mul(key, st["dh"], cx.dm[l, 3]), fr)
    elif name == "down":
        dd = st["gq"] if cx.dm else st["dh"]
        linear_bwd(dd, z["act"], sd[p + "ffn.net.3.weight"], fr, f"g:{p}ffn.net.3.bias", f"g:{p}ffn.net.3.weight", "da")
    elif name == "upre":
        put("xn", A.rms_rows(key, z["h2"], cx.gain(l, "norm3"), cx.mod(l, 1).repeat_interleave(T, 0)), fr)
        put("big", A.linear(key, own("xn"), sd[p + "ffn.net.0.weight"], sd[p + "ffn.net.0.bias"]), fr)
    elif name == "swiglu":
        put("big", A.swiglu_bwd(key, st["big"], st["da"], cx.dm.get((l, 2))), fr)
    elif name == "up":
        linear_bwd(st["big"], st["xn"], sd[p + "ffn.net.0.weight"], fr, f"g:{p}ffn.net.0.bias", f"g:{p}ffn.net.0.weight", "ga")
    elif name == "n3":
        norm_bwd("rms", z["h2"], st["ga"], cx.gain(l, "norm3"), cx.mod(l, 1), st["dh"], fr, B, "dh", cx.gain_name(l, "norm3"), None, (l, 1))
    elif name == "op":
        linear_bwd(st["dh"], z["att2"], sd[p + "cross_attn.out_proj.weight"], fr, None, f"g:{p}cross_attn.out_proj.weight", "ga")
    elif name == "cross":
        k, v = (z["kv"][:, i * H:(i + 1) * H].reshape(B, S, H) for i in range(2))
        r = attn(z["qc"].reshape(B, T, H), k, v, z["att2"].reshape(B, T, H), st["ga"].reshape(B, T, H), z["lse2"].reshape(B, cx.heads, T),
                 None, cx.cs.t_len, cx.cs.s_len, cx.dm.get((l, 1)))
        put("gq", r["dq"], fr, "zero")
        bar = None if r["dk"][1] is None else torch.cat([r["dk"][1], r["dv"][1]], 1)
        put("dkv", (torch.cat([r["dk"][0], r["dv"][0]], 1), bar), tk, "zero")
    elif name == "qp":
        put("xn", A.rms_rows(key, z["h1"], sd[p + "norm2.weight"], None), fr)
        linear_bwd(st["gq"], own("xn"), sd[p + "cross_attn.q_proj.weight"], fr, None, f"g:{p}cross_attn.q_proj.weight", "ga")
    elif name == "n2":
        norm_bwd("rms", z["h1"], st["ga"], sd[p + "norm2.weight"], None, st["dh"], fr, B, "dh", f"g:{p}norm2.weight")
    elif name == "kvu":
        put("crn", A.rms_rows(key, z["crp"], sd[p + "cross_attn.kv_norm.weight"], None), tk)
        linear_bwd(st["dkv"], own("crn"), sd[p + "cross_attn.kv_up_proj.weight"], tk, None, f"g:{p}cross_attn.kv_up_proj.weight", "dcr")
    elif name == "kvn":
        norm_bwd("rms", z["crp"], st["dcr"], sd[p + "cross_attn.kv_norm.weight"], None, None, tk, B, "dcp", f"g:{p}cross_attn.kv_norm.weight")
    elif name == "kvd":
        pre = st["dctx"]
        if isinstance(A, Emu) and A._m("dctx_last", key):
            pre = torch.zeros_like(pre)
        linear_bwd(st["dcp"], tp["ctx"], sd[p + "cross_attn.kv_down_proj.weight"], tk, None, f"g:{p}cross_attn.kv_down_proj.weight", "dctx", pre)
    elif name == "proj":
        linear_bwd(st["dh"], z["att1"], sd[p + "attn.proj.weight"], fr, f"g:{p}attn.proj.bias", f"g:{p}attn.proj.weight", "ga")
    elif name == "self":
        q, k, v = (z["qkv"][:, i * H:(i + 1) * H].reshape(B, T, H) for i in range(3))
        r = attn(q, k, v, z["att1"].reshape(B, T, H), st["ga"].reshape(B, T, H), z["lse1"].reshape(B, cx.heads, T), cx.cs.cfg.attn_window_size,
                 cx.cs.t_len, cx.cs.t_len, cx.dm.get((l, 0)))
        bar = None if r["dq"][1] is None else torch.cat([r[n][1] for n in ("dq", "dk", "dv")], 1)
        put("big", (torch.cat([r[n][0] for n in ("dq", "dk", "dv")], 1), bar), fr, "zero")
    elif name == "qkv":
        put("xn", A.rms_rows(key, z["h0"], cx.gain(l, "norm1"), cx.mod(l, 0).repeat_interleave(T, 0)), fr)
        linear_bwd(st["big"], own("xn"), sd[p + "attn.qkv.weight"], fr, None, f"g:{p}attn.qkv.weight", "ga")
    elif name == "n1":
        norm_bwd("rms", z["h0"], st["ga"], cx.gain(l, "norm1"), cx.mod(l, 0), st["dh"], fr, B, "dh", cx.gain_name(l, "norm1"), None, (l, 0))
    elif name == "inp":
        linear_bwd(st["dh"], cx.x, sd["in_proj.weight"], fr, "g:in_proj.bias", "g:in_proj.weight", "d_x")
    elif name == "sem":
        if cx.feats:
            linear_bwd(st["dctx"], cx.f, sd["sem_proj.weight"], tk, "g:sem_proj.bias", "g:sem_proj.weight", "d_sem")
        else:
            put("g:token_emb.weight", A.scatter(key, cx.cs.inp["sem"].reshape(-1), st["dctx"], cx.cs.cfg.codebook_size, tk))
    elif name == "ada":
        dm = st["dmod"].reshape(B, L, 2, 2 * H)
        dtc = torch.zeros(B, H, dtype=F64)
        bar = torch.zeros(B, H, dtype=F64)
        for ll in range(L):
            for which, nm in ((0, "norm1"), (1, "norm3")):
                pw = f"layers.{ll}.{nm}.proj."
                put("g:" + pw + "bias", A.colsum(key, dm[:, ll, which], _all(B)))
                put("g:" + pw + "weight", A.dw(key, dm[:, ll, which], tp["tcond"], _all(B)))
                r, b_ = A.dx(key, dm[:, ll, which], sd[pw + "weight"], None, dtc)
                dtc = r
                bar = None if b_ is None else bar + b_
        put("dtc", (dtc, bar))
    elif name == "step":
        put("g:step_emb.weight", A.scatter(key, cx.cs.inp["si"], st["dtc"], sd["step_emb.weight"].shape[0], _all(B)))
    elif name == "time":
        freqs = O.time_frequencies(H)
        put("e", A.time_emb(key, cx.cs.inp["t"], freqs))
        put("a1", A.linear(key, own("e"), sd["time_emb.1.weight"], sd["time_emb.1.bias"]))
        put("u1", A.gelu(key, own("a1")))
        put("g:time_emb.3.bias", A.colsum(key, st["dtc"], _all(B)))
        put("g:time_emb.3.weight", A.dw(key, st["dtc"], own("u1"), _all(B)))
        du = A.dx(key, st["dtc"], sd["time_emb.3.weight"], None)
        g_r, g_b = A.gelu_grad(key, du[0], own("a1"))
        if du[1] is not None:  # (the product's bar carried through the multiplication by GELU')
            cdf = 0.5 * (1 + torch.erf(own("a1") / math.sqrt(2.0)))
            g_b = g_b + du[1] * (cdf + (own("a1") * torch.exp(-0.5 * own("a1") ** 2) / math.sqrt(2 * math.pi)).abs())
        put("du1", (g_r, g_b))
        d1 = out["du1"].ref if got is None else got["du1"]
        put("g:time_emb.1.bias", A.colsum(key, d1, _all(B)))
        put("g:time_emb.1.weight", A.dw(key, d1, own("e"), _all(B)))
    else:
        raise KeyError(name)
    return out


OWN_SITES = ("out", "upre", "cross", "qp", "kvu", "self", "qkv", "time")


def site_id(key):
    l, name = key
    return f"L{l}.{name}" if name in LAYER else name


def chain(cx, A=None):
    """The final state of a whole backward, each site fed by the ones before it (A: a backend; default the fp64 references)."""
    A = A or Ref(cx)
    st = {}
    for key in cx.sites():
        for nm, o in _site(cx, key, st, A).items():
            st[nm] = o.ref
    return st


Result = collections.namedtuple("Result", "ratio worst_err worst_bar unwritten dead_nonzero")


def _compare(nm, o, got):
    assert got.shape == o.ref.shape, (nm, got.shape, o.ref.shape)
    ref, bar, g, dead_bad = o.ref, o.bar, got, 0
    if o.live is not None:
        sel = o.live if o.live.dim() == 2 else o.live[:, None].expand_as(ref)
        if o.dead == "zero":
            dead_bad = int((got[~sel] != 0).sum())  # (NaN counts)
        ref, bar, g = ref[sel], bar[sel], got[sel]
    ref, bar, g = ref.reshape(-1), bar.reshape(-1), g.reshape(-1)
    assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(bar).all()) and bool((bar >= 0).all()), nm
    fin = torch.isfinite(g)
    err = torch.where(fin, (g - ref).abs(), torch.zeros_like(ref))
    ratio = (err / bar.clamp_min(1e-300)).masked_fill(err == 0, 0.0)
    if not ratio.numel():
        return Result(0.0, 0.0, 0.0, 0, dead_bad)
    i = int(ratio.argmax())
    return Result(float(ratio[i]), float(err[i]), float(bar[i]), int((~fin).sum()), dead_bad)


def audit(cx, producer, amb=None, measure=None):
    """{(site id, output): Result}.  producer(key, st, shapes) -> {name: fp64 tensor}: what the audited run wrote at site `key` when
    the sites before it left `st` (shapes: {output name: its shape}).  The state handed on is the audited run's own."""
    ref = Ref(cx, amb, measure)
    st, res = {}, {}
    for key in cx.sites():
        outs = _site(cx, key, st, ref)
        got = producer(key, st, {nm: tuple(o.ref.shape) for nm, o in outs.items()})
        if key[1] in OWN_SITES:  # (the sites that read what they wrote: once more, on the audited run's own values)
            outs = _site(cx, key, st, Ref(cx), got)
        for nm, o in outs.items():
            res[site_id(key), nm] = _compare(nm, o, got[nm])
        st = dict(st)
        st.update(got)
    return res


def emulated(cx, mutant=None):
    """A producer: the fp32 emulation (with one mutant at its site)."""
    at = None
    if mutant is not None:
        site, which, _, _ = MUTANTS[mutant]
        at = (cx.L - 1 if which == "last" and site in LAYER else 0, site)
    emu = Emu(cx, mutant, at)
    return lambda key, st, shapes: {nm: o.ref for nm, o in _site(cx, key, st, emu).items()}


def mutant_target(cx, mutant):
    site, which, outp, _ = MUTANTS[mutant]
    l = cx.L - 1 if which == "last" and site in LAYER else 0
    return site_id((l, site)), outp.format(l=l)


def report(res, what):
    """Prints every site's worst error / bar over its outputs -- one line for the head, one per layer, one for the tail, then the worst
    of every site name over the layers -- and returns the latter as {site name: ratio}."""
    rows, by = {}, {}
    for (site, nm), r in res.items():
        group, _, stage = site.rpartition(".")
        group = group or ("head" if stage in HEAD else "tail")
        rows.setdefault(group, {})
        rows[group][stage] = max(rows[group].get(stage, 0.0), r.ratio)
        by[stage] = max(by.get(stage, 0.0), r.ratio)
    for group, stages in rows.items():
        print(f"{what} {group}: " + " ".join(f"{c} {v:.3f}" for c, v in stages.items()))
    print(f"{what}: " + " ".join(f"{c} {v:.3f}" for c, v in by.items()))
    return by


def check(res, what):
    by = report(res, what)
    bad = {k: v for k, v in res.items() if v.unwritten or v.dead_nonzero or not v.ratio <= 1.0}
    assert not bad, f"{what}: {bad}"
    return by


def measure_allowances(names):
    """{allowance: the fp32 CPU evaluation's worst error against fp64} BEFORE the margin, over the fp64 chains of the cases."""
    m = {}
    for name in names:
        cs = TA.case(name)
        cx = Ctx(cs, TA.OPTION_SETS[0], TA.chain(cs))
        chain(cx, Ref(cx, measure=m))
    return m  # (ETA_B is relative, the others are in units of u)
