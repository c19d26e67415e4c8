"""Shared by tests/test_hubert_audit_host.py and tests/test_hubert_audit_gpu.py: the site-by-site audit of the HuBERT backbone
(DESIGN.md section 35).  edtts_hubert_forward_until stops the forward after any site of its launch list, so each site's output is read
where it lies (native.hubert_workspace_views) and compared element by element with an fp64 evaluation of the same site, from the
operands that the runs stopped at the sites before it left behind and from the STATE DICT's weights (not the packed blob: the
transposes of the packing, the q | k | v concatenation and the bf16 rounding of the weights are audited with the first GEMM that reads
them).  The bars are sums of derived terms (u = 2^-24), section 29's where they exist (tape_audit_util):

  GEMM       K u sum_k |a_k||w_k| (any summation order of products), 2 u |partial| per epilogue add (bias, residual)
  GELU       an input bar e becomes 1.13 e (|gelu'| <= 1.13) + C_GELU u |x|: the kernels evaluate 0.5 x (1 + erff(x / sqrt 2)), whose
             error is absolute in erf, i.e. relative to |x| and not to |gelu(x)| in the negative tail
  norm       ETA ((|x| + |mean| + mean_k |x_k|) rstd |w| + |b|): section 29's summands and the row's mean magnitude, which is what the
             rounding error of an fp32 mean scales with (here rows follow a LayerNorm'd residual: mean ~ 0, elements near 0)
  GroupNorm  conv0's k0 u sum|w||x| carried to first order through the fp64 mean and variance, 2 u for the fp32 stores
  attention  ((n_i + 2) u [+ 2^-8 under bf16]) sum_j p_j |V_jd| + the score term (tape_audit_util.attention)
  storage    half a bf16 ulp at |ref| + bar where the site stores bf16
  exact      LENS (integers), VT (a permutation), ZERO, conv0's rows past an utterance's count

Under bf16 the reference rounds the weights itself; an activation operand is either stored as bf16 (read exactly) or the stored fp32
output of an earlier site that the GEMM rounds in staging (rnd(stored) is exact): no operand is recomputed by the kernel, so section
29's "ambiguous element" class does not arise.  ETA and C_GELU are train_util.MARGIN times the fp32 CPU evaluation's own worst error
against fp64 on the audit operands (measure_allowances; the host test asserts it).  Nothing here is fitted to what the kernels give.

A "snap" below is a dict {(site, index): fp64 tensor shaped as the site's output}."""
import collections
import functools
import json
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

import tape_audit_util as AT
from edge_diffusion_tts_amd import NativeHubert
from edge_diffusion_tts_amd.hubert import _POS_G, _POS_V
from train_util import MARGIN

F64, F32 = torch.float64, torch.float32
u = AT.u
ETA = 2.0 ** -20  # LayerNorm rows, relative to norm_rows' summands (MARGIN x measured, up to a power of two)
C_GELU = 8.0      # 0.5 x (1 + erf(x / sqrt 2)) in fp32, in units of u |x| (MARGIN x measured, up to a power of two)
GELU_SLOPE = 1.13  # max |gelu'| = 1.1289...
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hubert_small.npz")
FE = "feature_extractor.conv_layers."
E1_CONV = dict(conv_dim=(16, 24, 40), conv_kernel=(10, 3, 2), conv_stride=(5, 2, 2))

# name -> transformers-style config fields (the fixture's come from its file)
CONFIGS = {
    "E1": dict(E1_CONV, hidden_size=64, num_attention_heads=2, intermediate_size=136, num_conv_pos_embeddings=16,
               num_conv_pos_embedding_groups=4, num_hidden_layers=2),
    "E2": dict(conv_dim=(20, 12, 36), conv_kernel=(7, 3, 3), conv_stride=(3, 2, 1), hidden_size=72, num_attention_heads=3,
               intermediate_size=100, num_conv_pos_embeddings=5, num_conv_pos_embedding_groups=2, num_hidden_layers=1),
    "E3": dict(E1_CONV, hidden_size=96, num_attention_heads=1, intermediate_size=96, num_conv_pos_embeddings=4,
               num_conv_pos_embedding_groups=1, num_hidden_layers=1),
    "E4": dict(E1_CONV, hidden_size=128, num_attention_heads=1, intermediate_size=128, num_conv_pos_embeddings=4,
               num_conv_pos_embedding_groups=1, num_hidden_layers=1),
    # not in the issue's table: head_dim 64, the one k_hub_attn16 instance (<2>) the cases above leave out
    "E5": dict(E1_CONV, hidden_size=64, num_attention_heads=1, intermediate_size=64, num_conv_pos_embeddings=4,
               num_conv_pos_embedding_groups=1, num_hidden_layers=1),
    "A1": dict(conv_dim=(8, 72), conv_kernel=(10, 3), conv_stride=(5, 2), hidden_size=8, num_attention_heads=1, intermediate_size=8,
               num_conv_pos_embeddings=1, num_conv_pos_embedding_groups=1, num_hidden_layers=0),
}
SEEDS = {"E1": 101, "E2": 102, "E3": 103, "E4": 104, "A1": 105, "E5": 106}
ECASES = ("E1", "E2", "E3", "E4", "E5")
BF16_LEGAL = ("F", "E1", "E3", "E4", "E5")  # E2: conv_dim 20 / 12 / 36, head_dim 24; A1: head_dim 8
GN_T0 = (5, 255, 256, 257, 512, 513)  # conv0 frame counts around kGnChunk (E1; 5 is the stack's minimum: 4 frames leave no output frame)

Case = collections.namedtuple("Case", "name cfg sd layers C K S H heads DH I pk pg Cg eps")
Shape = collections.namedtuple("Shape", "tag wav lengths until")  # until: the last audited (site, index) or None for the whole forward


def redraw(model, seed):
    """Every parameter from a seeded generator (as tests/test_hubert_gpu.py and tests/golden/make_golden_hubert.py)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if "original0" in name or name.endswith("weight_g"):
                v = 1.0 + 2.0 * torch.rand(p.shape, generator=g)
            elif p.dim() == 1 and name.endswith("weight"):
                v = 1.0 + 0.2 * torch.randn(p.shape, generator=g)
            elif p.dim() == 1:
                v = 0.1 * torch.randn(p.shape, generator=g)
            else:
                v = torch.randn(p.shape, generator=g) / p[0].numel() ** 0.5
            p.copy_(v)
    return model


def fixture():
    z = np.load(GOLDEN)
    cfg = json.loads(bytes(z["config"]).decode())
    sd = {k[2:]: torch.from_numpy(z[k].astype(np.float32)) for k in z.files if k.startswith("w:")}
    return z, cfg, sd


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "F":
        _, cfg, sd = fixture()
        m = NativeHubert(cfg, cfg["num_hidden_layers"])
        m.load_state_dict(sd)
    else:
        cfg = CONFIGS[name]
        m = redraw(NativeHubert(cfg, cfg["num_hidden_layers"]), SEEDS[name])
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    H, heads = cfg["hidden_size"], cfg["num_attention_heads"]
    pg = cfg["num_conv_pos_embedding_groups"]
    return Case(name, cfg, sd, cfg["num_hidden_layers"], tuple(cfg["conv_dim"]), tuple(cfg["conv_kernel"]), tuple(cfg["conv_stride"]), H,
                heads, H // heads, cfg["intermediate_size"], cfg["num_conv_pos_embeddings"], pg, H // pg, 1e-5)


def module(cs, compute_dtype="fp32", num_layers=None):
    """A NativeHubert with the case's parameters (CPU; the caller moves it)."""
    m = NativeHubert(cs.cfg, cs.layers if num_layers is None else num_layers, compute_dtype=compute_dtype)
    m.load_state_dict(cs.sd)
    return m.eval()


# ------------------------------------------------------------------------------------------------------------ geometry
def stage_frames(cs, n):
    """Frames after every conv stage of n samples (an int or an int64 tensor)."""
    out = []
    for k, s in zip(cs.K, cs.S):
        n = (n - k) // s + 1
        out.append(n)
    return out


def samples_for(cs, frames):
    """The fewest samples that give `frames` output frames (the inverse recurrence)."""
    r = frames
    for k, s in zip(reversed(cs.K), reversed(cs.S)):
        r = (r - 1) * s + k
    return r


def _wav(B, T_audio, seed):
    return 0.1 * torch.randn(B, T_audio, generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=None)
def shapes(name):
    """The audited calls of a case: (tag, wav, lengths or None, last audited site or None)."""
    cs = case(name)
    if name == "F":
        z, _, _ = fixture()
        wav = torch.from_numpy(z["wav"].astype(np.float32))
        return (Shape("pad", wav, None, None), Shape("ragged", wav, torch.from_numpy(z["lengths"]).clone(), None))
    if name == "A1":  # conv1: M = 8100 frames x B = 8: ceil(8100 / 128) x 1 x 8 = 512 tiles of 128, N = 72 > 64; 64 GroupNorm chunks
        return (Shape("b8", _wav(8, samples_for(cs, 8100), 8100), None, ("conv", 1)),)
    seed = SEEDS[name] * 1000
    n1, n33, n65 = (samples_for(cs, t) for t in (1, 33, 65))
    wav = _wav(4, n65, seed + 65)
    lens = torch.tensor([n65, n65 + 7, n33, n1 - 5])
    for b, L in enumerate(lens.tolist()):
        if L < n65:
            wav[b, max(L, n1):] = float("nan") if b % 2 else 1e4  # (row 3 is clamped up to n1 samples: those are read)
    out = [Shape("t1", _wav(1, n1, seed + 1), None, None), Shape("ragged", wav, lens, None),
           Shape("t130", _wav(2, samples_for(cs, 130), seed + 130), None, None)]
    if name == "E1":
        out += [Shape(f"gn{t0}", _wav(2, (t0 - 1) * cs.S[0] + cs.K[0], seed + t0), None, ("conv0", 0)) for t0 in GN_T0]
    return tuple(out)


def site_list(cs, bf, with_lengths, until=None):
    """[(site, index)] in launch order, up to and including `until`."""
    out = ([("lens", 0)] if with_lengths else []) + [("gnstat", 0), ("conv0", 0)] + [("conv", i) for i in range(1, len(cs.C))]
    out += [("fpnorm", 0), ("fproj", 0), ("pos", 0), ("encnorm", 0)]
    for l in range(cs.layers):
        out += [(s, l) for s in ("qkv", "vt", "attn", "oproj", "ln1", "ff1", "ff2", "ln2") if bf or s != "vt"]
    if with_lengths:
        out.append(("zero", 0))
    return out[:out.index(tuple(until)) + 1] if until else out


def last_norm(cs):
    return ("ln2", cs.layers - 1) if cs.layers else ("encnorm", 0)


# ------------------------------------------------------------------------------------------------------------ layouts
LAYOUT_GOLDEN = os.path.join(os.path.dirname(GOLDEN), "hubert_layout.json")


def layout_records():
    """What the library's size queries answer (no GPU): {"case dtype BxT_audio": {"packed": bytes, "workspace": bytes, "regions":
    {member: [offset, bytes]}}} for every case at its first three shapes and hubert-base (nine layers) at 16 x 160000, in every
    compute dtype the case is legal in.  tests/golden/hubert_layout.json holds what the library answered before its two host-side
    descriptions (one per dtype) became one (tests/golden/make_hubert_layout.py)."""
    from edge_diffusion_tts_amd import native
    with torch.device("meta"):
        base = NativeHubert({}, 9).dims
    calls = [(name, module(case(name)).dims, [tuple(sh.wav.shape) for sh in shapes(name)[:3]]) for name in ("F",) + ECASES + ("A1",)]
    calls.append(("base9", base, [(16, 160000)]))
    out = {}
    for name, d, bts in calls:
        for dtype, dt in native.HUBERT_DTYPES.items():
            if dt and name not in BF16_LEGAL + ("base9",):
                continue
            for B, T_audio in bts:
                regs = {n: list(native.hubert_workspace_region(d, B, T_audio, dt, n)) for n in native.HUB_WS_REGIONS[:8 + dt]}
                out[f"{name} {dtype} {B}x{T_audio}"] = {"packed": native.hubert_packed_bytes(d, dt),
                                                        "workspace": native.hubert_workspace_bytes(d, B, T_audio, dt), "regions": regs}
    return out


# ------------------------------------------------------------------------------------------------------------ small pieces
def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x * math.sqrt(0.5)))


def gelu_bar(x, e):
    """The bar of gelu(x) for x known to +- e."""
    return GELU_SLOPE * e + C_GELU * u * x.abs()


def stored16(ref, bar, on):
    return bar + AT.half_ulp_bf16(ref.abs() + bar) if on else bar


def rows_lt(n, T):
    """[B, T, 1] bool: row t of utterance b is below n[b]."""
    return (torch.arange(T)[None, :] < n[:, None])[..., None]


def conv_gemm(x, w, rnd, stride=1, padding=0, groups=1):
    """x [B, T, C], w [co][ci / groups][k] (state-dict order) -> (the conv [B, T', co], its accumulation bar K u sum|a||w|)."""
    a, w = rnd(x).transpose(1, 2), rnd(w)
    K = w.shape[1] * w.shape[2]
    y = F.conv1d(a, w, stride=stride, padding=padding, groups=groups)
    e = (K * u) * F.conv1d(a.abs(), w.abs(), stride=stride, padding=padding, groups=groups)
    return y.transpose(1, 2), e.transpose(1, 2)


def dense(x, w, rnd):
    """x [B, T, K], w [N][K] -> (x w^T, K u |x||w|^T)."""
    y, e = AT.gemm(x.reshape(-1, x.shape[-1]), w, rnd)
    return y.reshape(*x.shape[:-1], -1), e.reshape(*x.shape[:-1], -1)


def norm_rows(x, w, b, eps):
    """(LayerNorm rows, their bar).  Section 29's summands (|x| + |mean|) rstd |w| + |b| plus the row's mean magnitude: an fp32 mean
    errs by a multiple of u mean_k |x_k| whatever |mean| is, and that error reaches every element of the row."""
    mu = x.mean(dim=-1, keepdim=True)
    rs = torch.rsqrt((x - mu).pow(2).mean(dim=-1, keepdim=True) + eps)
    return (x - mu) * rs * w + b, ETA * ((x.abs() + mu.abs() + x.abs().mean(dim=-1, keepdim=True)) * rs * w.abs() + b.abs())


def slot_key(p):
    """The key (inside its 32-key chunk) that slot p of k_hub_vt's layout holds (csrc/edtts_hubert16.h)."""
    return (16 if p & 4 else 0) + 4 * (p >> 3) + (p & 3)


def fold_pos(cs, dtype=F32):
    """The positional conv's weight with its weight norm folded in, in `dtype` (fp32: what NativeHubert hands to the packing)."""
    return torch._weight_norm(cs.sd[_POS_V].to(dtype), cs.sd[_POS_G].to(dtype), 2)


def fold_bar(cs):
    """|fp32 fold - fp64 fold| <= (n / 2 + 4) u |w|: a sum of n = H Cg squares in any order (n u relative), halved by the square root,
    and one rounding each for the square root, the product with g, the division and v's own square."""
    n = cs.H * cs.Cg
    return (n / 2 + 4) * u * fold_pos(cs, F64).abs()


def weights64(cs):
    return {k: v.to(F64) for k, v in cs.sd.items()}


def clean(v):
    """An operand as a contraction may read it: rows that no live element depends on may hold anything (the 0xFF fill, what the
    row-local steps made of the padding); they are made finite so that they stay in their rows."""
    return torch.nan_to_num(v, nan=0.0, posinf=0.0, neginf=0.0)


# ------------------------------------------------------------------------------------------------------------ the walk
def sites(cs, sh, bf, snap, pos_w=None, pre=None):
    """_sites up to and including the shape's last audited site."""
    for item in _sites(cs, sh, bf, snap, pos_w, pre):
        yield item
        if sh.until is not None and item[0] == tuple(sh.until):
            return


def _sites(cs, sh, bf, snap, pos_w, pre):
    """Yields ((site, index), class, reference, bar, live mask or None) for every audited site of the call in launch order, each
    from the operands that `snap` holds at that moment: a caller that stores the reference before asking for the next site chains
    the references (with bf False: the fp64 forward); one that stores what a run stopped there wrote audits the kernels.  Elements
    outside `live` may hold anything (nothing live reads them); where the kernels promise zeros the reference is 0 with bar 0.
    pos_w: the fp32 folded positional weight the packing was given (default: the CPU's fold).  pre: a dict that receives every GELU
    site's pre-activation."""
    sd, wav, lens = weights64(cs), sh.wav.to(F64), sh.lengths
    rnd = AT.bf16 if bf else AT.ident
    B, T_audio = wav.shape
    nc, H, L = len(cs.C), cs.H, cs.layers
    Ts = stage_frames(cs, T_audio)
    T, T0, C0 = Ts[-1], Ts[0], cs.C[0]
    def note(key, x):
        if pre is not None:
            pre[key] = x

    if lens is not None:
        fl = stage_frames(cs, lens.clamp(samples_for(cs, 1), T_audio))  # both clamps
        yield ("lens", 0), "exact", torch.stack([fl[0], fl[-1]]).to(F64), torch.zeros(2, B, dtype=F64), None
    else:
        fl = [torch.full((B,), t, dtype=torch.int64) for t in Ts]
    live = [rows_lt(fl[i], Ts[i]) for i in range(nc)]
    rows, flen = live[-1], fl[-1]
    k_len = None if lens is None else flen
    # conv0 in fp64 and its fp32 chain's bar; samples past a length are not operands (never read)
    read = torch.arange(T_audio)[None, :] < ((fl[0] - 1) * cs.S[0] + cs.K[0])[:, None]
    x0 = torch.where(read, wav, torch.zeros_like(wav))[:, None, :]
    w0 = sd[FE + "0.conv.weight"]
    v = F.conv1d(x0, w0, stride=cs.S[0]).transpose(1, 2)
    E = (cs.K[0] * u) * F.conv1d(x0.abs(), w0.abs(), stride=cs.S[0]).transpose(1, 2)
    m0 = live[0].to(F64)
    n0 = fl[0].to(F64)[:, None, None]
    mean = (v * m0).sum(1, keepdim=True) / n0
    var = ((v - mean).pow(2) * m0).sum(1, keepdim=True) / n0
    sc = sd[FE + "0.layer_norm.weight"] / torch.sqrt(var + 1e-5)
    sf = sd[FE + "0.layer_norm.bias"] - mean * sc
    d_mean = (E * m0).sum(1, keepdim=True) / n0
    d_var = 2.0 * ((v - mean).abs() * (E + d_mean) * m0).sum(1, keepdim=True) / n0
    d_sc = sc.abs() * d_var / (2.0 * (var + 1e-5))
    d_sf = sc.abs() * d_mean + mean.abs() * d_sc
    yield (("gnstat", 0), "groupnorm", torch.cat([sc, sf], 1), torch.cat([d_sc + 2 * u * sc.abs(), d_sf + 2 * u * sf.abs()], 1), None)
    st = snap["gnstat", 0]
    x = v * st[:, 0:1] + st[:, 1:2]
    note(("conv0", 0), x)
    ref, bar = gelu64(x), gelu_bar(x, E * st[:, 0:1].abs() + 2 * u * x.abs())
    bar = stored16(ref, bar, bf and nc > 1)
    yield ("conv0", 0), "conv0", torch.where(live[0], ref, torch.zeros_like(ref)), torch.where(live[0], bar, torch.zeros_like(bar)), None
    for i in range(1, nc):
        y, e = conv_gemm(clean(snap[("conv", i - 1) if i > 1 else ("conv0", 0)]), sd[f"{FE}{i}.conv.weight"], rnd, stride=cs.S[i])
        note(("conv", i), y)
        ref = gelu64(y)
        yield ("conv", i), "gemm+gelu", ref, stored16(ref, gelu_bar(y, e), bf and i + 1 < nc), live[i]
    feat = clean(snap[("conv", nc - 1) if nc > 1 else ("conv0", 0)])
    ref, bar = norm_rows(feat, sd["feature_projection.layer_norm.weight"], sd["feature_projection.layer_norm.bias"], cs.eps)
    yield ("fpnorm", 0), "norm", ref, bar, rows
    y, e = dense(clean(snap["fpnorm", 0]), sd["feature_projection.projection.weight"], rnd)
    yb = y + sd["feature_projection.projection.bias"]
    yield ("fproj", 0), "gemm", yb, e + AT.adds(yb), rows
    # h + GELU(pos_conv(h) + bias): zero rows outside [0, frames_b), the even kernel's last output dropped
    h = clean(snap["fproj", 0])
    wp = (fold_pos(cs) if pos_w is None else pos_w).to(F64)
    y, e = conv_gemm(torch.where(rows, h, torch.zeros_like(h)), wp, rnd, padding=cs.pk // 2, groups=cs.pg)
    yb = y[:, :T] + sd["encoder.pos_conv_embed.conv.bias"]
    note(("pos", 0), yb)
    gl = gelu64(yb)
    ref = h + gl
    yield ("pos", 0), "gemm+gelu", ref, gelu_bar(yb, e[:, :T] + AT.adds(yb)) + AT.adds(ref), rows
    ref, bar = norm_rows(clean(snap["pos", 0]), sd["encoder.layer_norm.weight"], sd["encoder.layer_norm.bias"], cs.eps)
    yield ("encnorm", 0), "norm", ref, bar, rows
    last = ("encnorm", 0)
    for l in range(L):
        p = f"encoder.layers.{l}."
        hin = clean(snap[last])
        w = torch.cat([sd[p + f"attention.{n}_proj.weight"] for n in "qkv"])
        b = torch.cat([sd[p + f"attention.{n}_proj.bias"] for n in "qkv"])
        y, e = dense(hin, w, rnd)
        yb = y + b
        yield ("qkv", l), "gemm", yb, stored16(yb, e + AT.adds(yb), bf), rows
        qkv = clean(snap["qkv", l])
        q, k, vv = (qkv[..., i * H:(i + 1) * H] for i in range(3))
        if bf:  # V^T [B][heads][DH][Tp] in slot order inside every 32-key chunk, zeros past the count, chunks past it not written
            Tp = (T + 31) // 32 * 32
            key = torch.tensor([32 * (j // 32) + slot_key(j % 32) for j in range(Tp)])
            vp = torch.cat([torch.where(rows, vv, torch.zeros_like(vv)), torch.zeros(B, Tp - T, H, dtype=F64)], 1)
            ref = vp[:, key].reshape(B, Tp, cs.heads, cs.DH).permute(0, 2, 3, 1)
            written = (32 * (torch.arange(Tp) // 32))[None, :] < flen[:, None]
            yield ("vt", l), "exact", ref, torch.zeros_like(ref), written[:, None, None, :].expand_as(ref)
        o, o_bar, _, _ = AT.attention(q, k, vv, cs.heads, None, k_len, rnd, bf, None)
        yield ("attn", l), "attention", o, stored16(o, o_bar, bf), rows
        y, e = dense(clean(snap["attn", l]), sd[p + "attention.out_proj.weight"], rnd)
        yb = y + sd[p + "attention.out_proj.bias"]
        yield ("oproj", l), "gemm", hin + yb, e + AT.adds(yb, hin + yb), rows
        ref, bar = norm_rows(clean(snap["oproj", l]), sd[p + "layer_norm.weight"], sd[p + "layer_norm.bias"], cs.eps)
        yield ("ln1", l), "norm", ref, bar, rows
        h1 = clean(snap["ln1", l])
        y, e = dense(h1, sd[p + "feed_forward.intermediate_dense.weight"], rnd)
        yb = y + sd[p + "feed_forward.intermediate_dense.bias"]
        note(("ff1", l), yb)
        ref = gelu64(yb)
        yield ("ff1", l), "gemm+gelu", ref, stored16(ref, gelu_bar(yb, e + AT.adds(yb)), bf), rows
        y, e = dense(clean(snap["ff1", l]), sd[p + "feed_forward.output_dense.weight"], rnd)
        yb = y + sd[p + "feed_forward.output_dense.bias"]
        yield ("ff2", l), "gemm", h1 + yb, e + AT.adds(yb, h1 + yb), rows
        ref, bar = norm_rows(clean(snap["ff2", l]), sd[p + "final_layer_norm.weight"], sd[p + "final_layer_norm.bias"], cs.eps)
        yield ("ln2", l), "norm", ref, bar, rows
        last = ("ln2", l)
    if lens is not None:
        src = snap[last]
        yield ("zero", 0), "exact", torch.where(rows, src, torch.zeros_like(src)), torch.zeros_like(src), None


def chain(cs, sh, bf=False, pos_w=None):
    """The snap of references, each site fed by the references before it: with bf False, the fp64 forward."""
    snap = {}
    for key, _, ref, _, _ in sites(cs, sh, bf, snap, pos_w):
        snap[key] = ref
    return snap


Result = collections.namedtuple("Result", "ratio worst_err worst_bar unwritten cls")


def judge(cls, got, ref, bar, live):
    """The worst error / bar over the live elements of one site and how many of them are not finite (not written)."""
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if live is not None:
        live = live.expand_as(ref)
        got, ref, bar = got[live], ref[live], bar[live]
    got, ref, bar = got.reshape(-1), ref.reshape(-1), bar.reshape(-1)
    assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(bar).all()) and bool((bar >= 0).all())
    if not got.numel():
        return Result(0.0, 0.0, 0.0, 0, cls)
    fin = torch.isfinite(got)
    err = torch.where(fin, (got - ref).abs(), torch.zeros_like(ref))
    ratio = (err / bar.clamp_min(1e-300)).masked_fill(err == 0, 0.0)
    i = int(ratio.argmax())
    return Result(float(ratio[i]), float(err[i]), float(bar[i]), int((~fin).sum()), cls)


def audit(cs, sh, bf, snap, pos_w=None):
    """{(site, index): Result} of a filled snap."""
    return {key: judge(cls, snap[key], ref, bar, live) for key, cls, ref, bar, live in sites(cs, sh, bf, snap, pos_w)}


def report(res, what):
    """Prints every site's worst error / bar (over its layers); returns {site: worst ratio}."""
    by = {}
    for (site, _), r in res.items():
        by[site] = max(by.get(site, 0.0), r.ratio)
    print(f"{what}: " + "  ".join(f"{s} {v:.3f}" for s, v in by.items()))
    return by


def check(res, what):
    by = report(res, what)
    bad = {k: v for k, v in res.items() if v.unwritten or not v.ratio <= 1.0}
    assert not bad, f"{what}: {bad}"
    return by


# ------------------------------------------------------------------------------------------------------------ the CPU's own error
NORM_PARAMS = {"fpnorm": "feature_projection.layer_norm.", "encnorm": "encoder.layer_norm.", "ln1": "encoder.layers.{}.layer_norm.",
               "ln2": "encoder.layers.{}.final_layer_norm."}


def gelu32(x):
    """The kernels' formula (csrc/edtts_hubert.h: gelu) in fp32."""
    return 0.5 * x * (1.0 + torch.erf(x * 0.70710678118654752440))


def measure_allowances(names):
    """(eta, c_gelu) BEFORE the margin: the fp32 CPU evaluation's worst error against fp64 on the fp32 operands that the fp64 chains of
    the cases produce (live elements).  eta: LayerNorm rows relative to their summands (norm_rows' bar / ETA); c_gelu: the
    kernels' formula 0.5 x (1 + erf(x 0.70710678...)) in fp32 on every GELU site's pre-activations, in units of u |x|."""
    eta = c_gelu = 0.0

    def worst(v, live):
        v = v if live is None else v[live.expand_as(v)]
        v = v[torch.isfinite(v)]
        return float(v.max()) if v.numel() else 0.0

    for name in names:
        cs = case(name)
        for sh in shapes(name):
            snap, pre, prev = {}, {}, None
            for key, cls, ref, _, live in sites(cs, sh, False, snap, pre=pre):
                snap[key] = ref
                if cls == "norm":
                    x32 = clean(snap[prev]).to(F32)
                    w, b = (cs.sd[NORM_PARAMS[key[0]].format(key[1]) + n] for n in ("weight", "bias"))
                    y32 = F.layer_norm(x32, (x32.shape[-1],), w, b, cs.eps)
                    y64, d = norm_rows(x32.to(F64), w.to(F64), b.to(F64), cs.eps)
                    eta = max(eta, worst((y32.to(F64) - y64).abs() / (d / ETA).clamp_min(1e-300), live))
                elif key in pre:
                    x32 = pre[key].to(F32)
                    x64 = x32.to(F64)
                    err = (gelu32(x32).to(F64) - gelu64(x64)).abs() / (u * x64.abs()).clamp_min(1e-300)
                    c_gelu = max(c_gelu, worst(err, rows_lt(torch.full((x32.shape[0],), x32.shape[1]), x32.shape[1]) if live is None else live))
                prev = key
    return eta, c_gelu


# ------------------------------------------------------------------------------------------------------------ an fp32 emulation
# One draw of what the contract allows, in fp32 torch: the fp32 path consumes K in chunks of 16, the bf16 path rounds both operands and
# consumes K in chunks of 32, its attention is an online softmax in 32-key steps with P rounded to bf16 against the running maximum.
# It shows that the bars can be met; its mutants, each a fault of the kind a kernel can have, show that they are not vacuous.
# name -> (case, shape tag, bf16?, the site whose bar must catch it)
MUTANTS = {
    "conv_layout": ("E1", "t130", False, ("conv", 1)),        # the conv weight left [co][ci][k]
    "k_term": ("E1", "t130", False, ("fproj", 0)),            # the k-term K - 1 dropped (K = 40: a tail under both K tiles)
    "k_term16": ("E1", "t130", True, ("fproj", 0)),
    "pos_pad": ("E1", "t130", False, ("pos", 0)),             # the positional conv padded by pk / 2 - 1
    "pos_row_flen": ("E1", "ragged", False, ("pos", 0)),      # ... reading row flen_b of a ragged utterance
    "group0": ("E1", "t130", False, ("pos", 0)),              # group g reading group 0's channels
    "even_last": ("E1", "t130", False, ("pos", 0)),           # the even kernel keeping the last frame (dropping the first)
    "gn_padded": ("E1", "ragged", False, ("gnstat", 0)),      # GroupNorm statistics over the padded T0 instead of len0
    "gn_last_chunk": ("E1", "gn513", False, ("gnstat", 0)),   # the last GroupNorm chunk (one frame of 513) dropped
    "no_gelu": ("E1", "t130", False, ("conv", 1)),            # GELU omitted at a conv
    "no_bias": ("E1", "t130", False, ("fproj", 0)),           # the bias omitted
    "snapshot": ("E1", "t130", False, ("ff2", 0)),            # the residual from the wrong snapshot (before LN1)
    "qkv_order": ("E1", "t130", False, ("qkv", 0)),           # k | q | v
    "key_at_len": ("E1", "ragged", False, ("attn", 0)),       # the key at index T_b read
    "key_at_len16": ("E1", "ragged", True, ("attn", 0)),
    "vt_unpermuted": ("E1", "t130", True, ("vt", 0)),         # V slots left in key order
    "unrounded": ("E1", "t130", True, ("fproj", 0)),          # the weights left unrounded under bf16
    "not_zeroed": ("E1", "ragged", False, ("zero", 0)),       # rows past the count not zeroed
}


def bf16_32(v):
    return v.to(torch.bfloat16).to(F32)


def fma32(a, b, c):
    """One rounding: fp32 products are exact in fp64."""
    return (a.to(F64) * b.to(F64) + c.to(F64)).to(F32)


def im2col(x, k, s, left=0, right=0):
    """x [B, T, C] -> [B, T', k C], tap-major (k = tap C + ci): the implicit GEMM's rows."""
    if left or right:
        x = F.pad(x, (0, 0, left, right))
    return x.unfold(1, k, s).permute(0, 1, 3, 2).reshape(x.shape[0], -1, k * x.shape[-1])


def emulate(cs, sh, bf, mutant=None):
    """The snap of an fp32 emulation of the call (fp64 tensors holding fp32 / bf16 values)."""
    sd = {k: v.to(F32) for k, v in cs.sd.items()}
    wav, lens = clean(sh.wav.to(F32)), sh.lengths
    B, T_audio = wav.shape
    nc, H, L, heads, DH = len(cs.C), cs.H, cs.layers, cs.heads, cs.DH
    Ts = stage_frames(cs, T_audio)
    T, T0 = Ts[-1], Ts[0]
    r, kc = (bf16_32, 32) if bf else (AT.ident, 16)
    snap = {}

    class Done(Exception):
        pass

    def put(key, v):
        snap[key] = v.to(F64)
        if sh.until is not None and key == tuple(sh.until):
            raise Done

    def mm(a, w, drop_last=False, rw=None):
        a, w = r(a), (rw or r)(w)
        K = a.shape[-1] - (1 if drop_last else 0)
        acc = torch.zeros(a.shape[0], w.shape[0], dtype=F32)
        for k0 in range(0, K, kc):
            acc = acc + a[:, k0:min(K, k0 + kc)] @ w[:, k0:min(K, k0 + kc)].T
        return acc

    def lin(x, w, b, **kw):
        y = mm(x.reshape(-1, x.shape[-1]), w, **kw).reshape(*x.shape[:-1], -1)
        return y if b is None else y + b

    def ln(x, name):
        return F.layer_norm(x, (x.shape[-1],), sd[name + "weight"], sd[name + "bias"], cs.eps)

    def st16(v, on=True):
        return bf16_32(v) if bf and on else v

    try:
        if lens is not None:
            fl = stage_frames(cs, lens.clamp(samples_for(cs, 1), T_audio))
            put(("lens", 0), torch.stack([fl[0], fl[-1]]))
        else:
            fl = [torch.full((B,), t, dtype=torch.int64) for t in Ts]
        flen = fl[-1]
        rows = rows_lt(flen, T)
        # conv0: an fp32 FMA chain over the taps; statistics in fp64 over the utterance's own frames
        w0, cols = sd[FE + "0.conv.weight"][:, 0, :], wav.unfold(1, cs.K[0], cs.S[0])
        v = torch.zeros(B, T0, cs.C[0], dtype=F32)
        for j in range(cs.K[0]):
            v = fma32(w0[:, j][None, None, :], cols[:, :, j:j + 1], v)
        n0 = torch.full_like(fl[0], T0) if mutant == "gn_padded" else fl[0]
        summed = n0 if mutant != "gn_last_chunk" else 256 * ((n0 - 1) // 256)
        m0, nf = rows_lt(summed, T0).to(F64), n0.to(F64)[:, None]
        s, q = (v.to(F64) * m0).sum(1) / nf, (v.to(F64).pow(2) * m0).sum(1) / nf
        sc = sd[FE + "0.layer_norm.weight"].to(F64) / torch.sqrt((q - s * s).clamp_min(0.0) + 1e-5)
        stats = torch.stack([sc, sd[FE + "0.layer_norm.bias"].to(F64) - s * sc], 1).to(F32)
        put(("gnstat", 0), stats)
        y = gelu32(fma32(v, stats[:, 0:1], stats[:, 1:2]))
        x = st16(torch.where(rows_lt(fl[0], T0), y, torch.zeros_like(y)), nc > 1)
        put(("conv0", 0), x)
        for i in range(1, nc):
            W = sd[f"{FE}{i}.conv.weight"]
            w2 = W.reshape(W.shape[0], -1) if (mutant == "conv_layout" and i == 1) else W.permute(0, 2, 1).reshape(W.shape[0], -1)
            y = lin(im2col(x, cs.K[i], cs.S[i]), w2, None)
            x = st16(y if (mutant == "no_gelu" and i == 1) else gelu32(y), i + 1 < nc)
            put(("conv", i), x)
        fn = ln(x, "feature_projection.layer_norm.")
        put(("fpnorm", 0), fn)
        h = lin(fn, sd["feature_projection.projection.weight"], None if mutant == "no_bias" else sd["feature_projection.projection.bias"],
                drop_last=mutant in ("k_term", "k_term16"), rw=AT.ident if mutant == "unrounded" else None)
        put(("fproj", 0), h)
        nv = (flen + 1).clamp(max=T) if mutant == "pos_row_flen" else flen
        hz = torch.where(rows_lt(nv, T), h, torch.zeros_like(h))
        wp, pad, first = fold_pos(cs), cs.pk // 2 - (1 if mutant == "pos_pad" else 0), 1 if mutant == "even_last" else 0
        ys = []
        for g in range(cs.pg):
            src = 0 if mutant == "group0" else g
            a = im2col(hz[..., src * cs.Cg:(src + 1) * cs.Cg], cs.pk, 1, pad, cs.pk + 1)[:, first:first + T]
            wg = wp[g * cs.Cg:(g + 1) * cs.Cg]
            ys.append(lin(a, wg.permute(0, 2, 1).reshape(cs.Cg, -1), sd["encoder.pos_conv_embed.conv.bias"][g * cs.Cg:(g + 1) * cs.Cg]))
        pos = h + gelu32(torch.cat(ys, -1))
        put(("pos", 0), pos)
        h = ln(pos, "encoder.layer_norm.")
        put(("encnorm", 0), h)
        for l in range(L):
            p, m = f"encoder.layers.{l}.", mutant if l == 0 else None
            order = "kqv" if m == "qkv_order" else "qkv"
            qkv = st16(lin(h, torch.cat([sd[p + f"attention.{n}_proj.weight"] for n in order]),
                           torch.cat([sd[p + f"attention.{n}_proj.bias"] for n in order])))
            put(("qkv", l), qkv)
            q, k, vv = (qkv[..., i * H:(i + 1) * H] for i in range(3))
            kl = (flen + 1).clamp(max=T) if m in ("key_at_len", "key_at_len16") else flen
            if bf:
                Tp = (T + 31) // 32 * 32
                key = torch.tensor([j if m == "vt_unpermuted" else 32 * (j // 32) + slot_key(j % 32) for j in range(Tp)])
                vp = torch.cat([torch.where(rows, vv, torch.zeros_like(vv)), torch.zeros(B, Tp - T, H)], 1)
                put(("vt", l), vp[:, key].reshape(B, Tp, heads, DH).permute(0, 2, 3, 1))
            qh, kh, vh = (z.reshape(B, T, heads, DH).transpose(1, 2) for z in (q, k, vv))
            ok = (torch.arange(T)[None, :] < kl[:, None])[:, None, None, :].expand(B, heads, T, T)
            if bf:
                scale = torch.tensor(1.4426950408889634 / math.sqrt(DH), dtype=F32)
                mx = torch.full((B, heads, T), -1e30, dtype=F32)
                lsum, acc = torch.zeros(B, heads, T, dtype=F32), torch.zeros(B, heads, T, DH, dtype=F32)
                for j0 in range(0, T, 32):
                    j1 = min(T, j0 + 32)
                    sc_ = ((qh @ kh[:, :, j0:j1].transpose(-1, -2)) * scale).masked_fill(~ok[..., j0:j1], float("-inf"))
                    mn = torch.maximum(mx, sc_.amax(dim=-1))
                    alpha, pj = torch.exp2(mx - mn), torch.exp2(sc_ - mn[..., None])
                    lsum = lsum * alpha + pj.sum(dim=-1)
                    acc = acc * alpha[..., None] + bf16_32(pj) @ vh[:, :, j0:j1]
                    mx = mn
                o = acc / lsum[..., None]
            else:
                sc_ = ((qh @ kh.transpose(-1, -2)) / math.sqrt(DH)).masked_fill(~ok, float("-inf"))
                o = torch.softmax(sc_, dim=-1) @ vh
            att = st16(o.transpose(1, 2).reshape(B, T, H))
            put(("attn", l), att)
            h0 = h
            h = h0 + lin(att, sd[p + "attention.out_proj.weight"], sd[p + "attention.out_proj.bias"])
            put(("oproj", l), h)
            h1 = ln(h, p + "layer_norm.")
            put(("ln1", l), h1)
            ff = st16(gelu32(lin(h1, sd[p + "feed_forward.intermediate_dense.weight"], sd[p + "feed_forward.intermediate_dense.bias"])))
            put(("ff1", l), ff)
            h = (h if m == "snapshot" else h1) + lin(ff, sd[p + "feed_forward.output_dense.weight"], sd[p + "feed_forward.output_dense.bias"])
            put(("ff2", l), h)
            h = ln(h, p + "final_layer_norm.")
            put(("ln2", l), h)
        if lens is not None:
            put(("zero", 0), h if mutant == "not_zeroed" else torch.where(rows, h, torch.zeros_like(h)))
    except Done:
        pass
    return snap
