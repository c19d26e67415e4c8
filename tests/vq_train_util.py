"""Shared by tests/test_vq_train_host.py, tests/test_vq_train_gpu.py and tests/golden/make_golden_train_vq.py: the VQ head
(proj -> VectorQuantizer in training mode) restated in plain torch -- differentiable, in any dtype, in the reference's exact order
(models/vq.py:70-145: the lookup, the two mse losses, the EMA update that overwrites the codebook inside the forward, the dead-code
reset with a given permutation, then the straight-through line) --, the training cases and their oracle results (fp64: the arbiter,
fp32: the yardstick), each computed once and never modified.

An argmin that differs between the fp32 and the fp64 oracle would inflate E_ref and hide a failure, so every case uses the first
feature seed >= 100 at which, in fp64, at every step and under each of its dropout seeds, the gap between the smallest and the
second smallest distance is >= MIN_GAP on every valid frame, and on a reset step every code's |ema_cluster_size - 1| is >= MIN_DEAD:
FEATURE_SEED below was searched on the CPU for that and tests/test_vq_train_host.py asserts it."""
import functools

import torch

import sem_train_util as SU
from dropout_util import seeds_of
from edge_diffusion_tts_amd.synth import _u, synth_hubert_features, synth_semantic_head
from train_util import MARGIN, rel_err  # noqa: F401  (re-exported)

MIN_GAP = 1e-3
MIN_DEAD = 1e-4
COMMIT, DECAY, EPSILON = 0.25, 0.99, 1e-5  # VectorQuantizer's defaults
LOSS_W = 10.0                              # the objective: (z_q . C).sum() + LOSS_W vq_loss
LR = 0.05                                  # the in-test SGD step of the multi-step runs
PROJ_KEYS = ("w1", "b1", "lng", "lnb", "w3", "b3")

# name -> (in_dim (0: VectorQuantizer alone), S, K, dropout p or None (None: the 4-module proj), B, T)
CASES = {
    "V1": (768, 128, 512, None, 2, 37),
    "V2": (256, 64, 1000, 0.2, 3, 50),
    "V3": (0, 32, 24, None, 2, 33),
    "V4": (128, 64, 64, None, 4, 175),
    "V5": (48, 16, 5, 0.5, 1, 5),
}
WEIGHT_SEED = {"V1": 1, "V2": 2, "V3": 3, "V4": 4, "V5": 5}
FEATURE_SEED = {"V1": 101, "V2": 100, "V3": 101, "V4": 101, "V5": 100}
DROP_GENS = {"V2": (11,), "V5": (11,)}
DROP_SEEDS = {k: tuple(seeds_of(g)[0] for g in v) for k, v in DROP_GENS.items()}
V2_LENGTHS = (50, 17, 1)
RESET_GEN = 31          # seed of the reset permutation's CPU generator in the multi-step runs
MULTI = ("V3", "V4")    # the cases of the three-step run (reset_unused_every = 2)


def param_names(in_dim, dropout_layout, prefix="vq."):
    """canonical name -> the parameter's name in SemanticEncoder (VectorQuantizer alone: prefix "")"""
    names = {"cb": prefix + "codebook.weight"}
    if in_dim:
        last = "4" if dropout_layout else "3"
        names.update(w1="proj.0.weight", b1="proj.0.bias", lng="proj.2.weight", lnb="proj.2.bias", w3=f"proj.{last}.weight", b3=f"proj.{last}.bias")
    return names


def start_buffers(K, S, cb, seed):
    """Deterministic non-trivial starting buffers: ema_cluster_size hash-uniform in [0.2, 3), ema_w away from the codebook."""
    ecs = 1.6 + _u((K,), seed, 140, 1.4)
    ema_w = cb * ecs[:, None] + _u((K, S), seed, 141, 0.05)
    return ecs.contiguous(), ema_w.contiguous()


@functools.lru_cache(maxsize=None)
def case(name, feature_seed=None):
    """(in_dim, S, K, p, B, T, proj state dict or None, quantizer state dict with the starting buffers, features, C [B, T, S])"""
    in_dim, S, K, p, B, T = CASES[name]
    proj_sd, q_sd = synth_semantic_head(in_dim or 16, S, None, codebook_size=K, seed=WEIGHT_SEED[name], dropout_layout=p is not None)
    fs = FEATURE_SEED[name] if feature_seed is None else feature_seed
    x = synth_hubert_features(B, T, in_dim or S, fs)
    if not in_dim:
        proj_sd, x = None, 0.9 * x
    q_sd = dict(q_sd)
    q_sd["ema_cluster_size"], q_sd["ema_w"] = start_buffers(K, S, q_sd["codebook.weight"], WEIGHT_SEED[name])
    C = torch.randn(B, T, S, generator=torch.Generator().manual_seed(B * 1000 + T))
    return in_dim, S, K, p, B, T, proj_sd, q_sd, x, C


def weights_of(proj_sd, q_sd):
    out = {}
    if proj_sd is not None:
        last = "4" if "4.weight" in proj_sd else "3"
        out.update(w1=proj_sd["0.weight"], b1=proj_sd["0.bias"], lng=proj_sd["2.weight"], lnb=proj_sd["2.bias"],
                   w3=proj_sd[last + ".weight"], b3=proj_sd[last + ".bias"])
    out["cb"] = q_sd["codebook.weight"]
    return out


def proj_forward(p, x, mult=None):
    F = torch.nn.functional
    a = F.layer_norm(F.gelu(F.linear(x, p["w1"], p["b1"])), (p["lng"].shape[0],), p["lng"], p["lnb"], 1e-5)
    if mult is not None:
        a = a * mult
    return F.linear(a, p["w3"], p["b3"])


class Head:
    """The head's state in one dtype: parameters (leaves), the three buffers, and VectorQuantizer.forward restated."""

    def __init__(self, w, q_sd, dtype, commit=COMMIT, decay=DECAY, epsilon=EPSILON, reset_unused_every=100):
        self.dtype = dtype
        self.p = {k: v.to(dtype).clone().requires_grad_(True) for k, v in w.items()}
        self.ecs = q_sd["ema_cluster_size"].to(dtype).clone()
        self.ema_w = q_sd["ema_w"].to(dtype).clone()
        self.count = int(q_sd["update_count"])
        self.commit, self.decay, self.epsilon, self.reset_unused_every = commit, decay, epsilon, reset_unused_every
        self.last = {}

    def quantize(self, z, training=True, perm=None):
        """z [N, S] -> (z_q, idx, vq_loss); in training mode the EMA update and the reset (perm: what torch.randperm(N) returns)
        change the state, after the loss was formed against the codebook as given."""
        F = torch.nn.functional
        C = self.p["cb"]
        K = C.shape[0]
        flat = z
        dist = flat.pow(2).sum(1, keepdim=True) - 2 * flat @ C.t() + C.pow(2).sum(1, keepdim=True).t()
        idx = dist.argmin(dim=1)
        two = torch.topk(dist.detach(), min(2, K), dim=1, largest=False).values
        self.last = dict(gap=(two[:, -1] - two[:, 0]) if K > 1 else torch.full((len(z),), float("inf")), reset=False, dead_margin=None, rows=None)
        c = C[idx]
        if training:
            vq_loss = F.mse_loss(c, z.detach()) + self.commit * F.mse_loss(c.detach(), z)
            if self.decay > 0:
                with torch.no_grad():
                    enc = F.one_hot(idx, K).to(self.dtype)
                    self.ecs.mul_(self.decay).add_(enc.sum(0), alpha=1 - self.decay)
                    self.ema_w.mul_(self.decay).add_(enc.t() @ flat.detach(), alpha=1 - self.decay)
                    C.data.copy_(self.ema_w / self.ecs.clamp_min(self.epsilon).unsqueeze(1))
                    self.count += 1
                    if self.reset_unused_every > 0 and self.count % self.reset_unused_every == 0:
                        dead = self.ecs < 1.0
                        self.last.update(reset=True, dead_margin=(self.ecs.double() - 1.0).abs().min())
                        num_dead = int(dead.sum())
                        if num_dead > 0 and flat.shape[0] > 0:
                            n = min(num_dead, flat.shape[0])
                            rows = perm(flat.shape[0])[:n]
                            di = dead.nonzero(as_tuple=True)[0][:n]
                            C.data[di] = flat.detach()[rows]
                            self.ema_w[di] = flat.detach()[rows]
                            self.ecs[di] = 1.0
                            self.last["rows"], self.last["dead"] = rows, di
        else:
            vq_loss = torch.zeros((), dtype=self.dtype)
        return z + (c - z).detach(), idx, vq_loss

    def step(self, x, Cw, loss_w=LOSS_W, with_zq=True, mult=None, lengths=None, training=True, perm=None, leaf=False):
        """One forward / backward of the objective (z_q . Cw).sum() [with_zq] + loss_w vq_loss on the valid frames (lengths: the
        utterances trimmed and concatenated).  Returns a dict: idx, zq, loss, gap, every gradient as "g.<name>" (+ "g.d_z"), the
        buffers and the codebook after the step as "ecs", "ema_w", "cb", the count, and the reset's rows."""
        for v in self.p.values():
            v.grad = None
        S = x.shape[-1] if "w1" not in self.p else self.p["w3"].shape[0]
        xx = x.to(self.dtype).clone()
        sel = None
        if lengths is not None:
            sel = torch.cat([torch.arange(n) + b * x.shape[1] for b, n in enumerate(lengths)])
        flat = lambda t: None if t is None else (t.reshape(-1, t.shape[-1]) if sel is None else t.reshape(-1, t.shape[-1])[sel])  # noqa: E731
        xf = flat(xx).requires_grad_(leaf)
        z = proj_forward(self.p, xf, flat(None if mult is None else mult.to(self.dtype))) if "w1" in self.p else xf
        zq, idx, loss = self.quantize(z, training, perm)
        obj = loss_w * loss
        if with_zq:
            obj = obj + (zq * flat(Cw.to(self.dtype))).sum()
        obj.backward()
        out = dict(idx=idx, zq=zq.detach(), loss=loss.detach(), gap=self.last["gap"], reset=self.last["reset"],
                   dead_margin=self.last["dead_margin"], rows=self.last["rows"], dead=self.last.get("dead"), count=self.count, sel=sel,
                   ecs=self.ecs.clone(), ema_w=self.ema_w.clone(), cb=self.p["cb"].detach().clone())
        for k, v in self.p.items():
            out["g." + k] = torch.zeros_like(v) if v.grad is None else v.grad.clone()
        if leaf:
            out["g.d_z"] = xf.grad.clone()
        assert S == zq.shape[-1]
        return out

    def sgd(self, lr=LR):
        with torch.no_grad():
            for v in self.p.values():
                if v.grad is not None:
                    v.data.sub_(lr * v.grad)


def multiplier(name, drop_seed, dtype):
    in_dim, S, K, p, B, T = CASES[name]
    return None if drop_seed is None else SU.head_multiplier(drop_seed, p, B, T, S, dtype)


def fixed_perm(gen_seed):
    """perm(N) -> torch.randperm(N) from one CPU generator seeded once: what a module whose reset_generator was seeded alike draws"""
    g = torch.Generator().manual_seed(gen_seed)
    return lambda n: torch.randperm(n, generator=g)


@functools.lru_cache(maxsize=None)
def run(name, dtype, steps=1, drop_seed=None, lengths=None, with_zq=True, training=True, reset_unused_every=100, sgd=False, feature_seed=None):
    """The case's `steps` consecutive forwards / backwards (sgd: an SGD update of every parameter after each): a list of Head.step
    results."""
    in_dim, S, K, p, B, T, proj_sd, q_sd, x, C = case(name, feature_seed)
    head = Head(weights_of(proj_sd, q_sd), q_sd, dtype, reset_unused_every=reset_unused_every)
    perm = fixed_perm(RESET_GEN)
    out = []
    for s in range(steps):
        out.append(head.step(x, C, with_zq=with_zq, mult=multiplier(name, drop_seed, dtype), lengths=lengths, training=training, perm=perm,
                             leaf=not in_dim))
        if sgd:
            head.sgd()
    return out


FLOAT_KEYS = ("loss", "ecs", "ema_w", "cb")


def variants(name):
    """The keyword sets of run() that the GPU tests compare against: the margin conditions must hold in every one."""
    v = [dict(steps=2)]
    v += [dict(drop_seed=s) for s in DROP_SEEDS.get(name, ())]
    if name == "V2":
        v += [dict(lengths=V2_LENGTHS), dict(lengths=V2_LENGTHS, drop_seed=DROP_SEEDS["V2"][0])]
    if name in MULTI:
        v.append(dict(steps=3, reset_unused_every=2, sgd=True))
    return v


def margins(name, feature_seed=None):
    """(smallest fp64 distance gap over every variant, step and frame; smallest |ema_cluster_size - 1| over the reset steps or None;
    fp32 and fp64 idx equal everywhere)"""
    gap, dead, same = float("inf"), None, True
    for kw in variants(name):
        r64 = run(name, torch.float64, feature_seed=feature_seed, **kw)
        r32 = run(name, torch.float32, feature_seed=feature_seed, **kw)
        for a, b in zip(r64, r32):
            gap = min(gap, float(a["gap"].min()))
            same = same and torch.equal(a["idx"], b["idx"])
            if a["reset"]:
                dead = float(a["dead_margin"]) if dead is None else min(dead, float(a["dead_margin"]))
    return gap, dead, same


def oracle(name, **kw):
    """(fp64 results per step, fp32 results per step, E_ref per step {key: E}, median E_ref per step)"""
    r64, r32 = run(name, torch.float64, **kw), run(name, torch.float32, **kw)
    e_refs, meds = [], []
    for a, b in zip(r64, r32):
        e = {k: rel_err(b[k], a[k]) for k in a if (k.startswith("g.") or k in FLOAT_KEYS) and float(a[k].abs().max()) > 0}
        e_refs.append(e)
        meds.append(float(torch.tensor(sorted(e.values())).median()))
    return r64, r32, e_refs, meds


def check(got, ref64, e_ref, med, what, keys=None):
    """`got`: {key: tensor}.  Every entry within the bar E <= MARGIN * max(E_ref, median E_ref) of ref64 (an all-zero reference: exactly
    zero); returns the worst ratio after printing every one."""
    worst, bad = 0.0, []
    for k in (sorted(got) if keys is None else keys):
        v = ref64[k]
        assert got[k] is not None, f"{what}: {k} is missing"
        assert tuple(got[k].shape) == tuple(v.shape), (k, got[k].shape, v.shape)
        if float(v.abs().max()) == 0:
            assert not bool(got[k].any()), f"{what}: {k} must be exactly zero"
            continue
        e = rel_err(got[k], v)
        bar = max(e_ref[k], med)
        ratio = e / bar if bar > 0 else (0.0 if e == 0 else float("inf"))  # (both oracles exact: so must the result be)
        print(f"{what} {k}: E {e:.2e}  E_ref {e_ref[k]:.2e}  ratio {ratio:.2f}")
        worst = max(worst, ratio)
        if not e <= MARGIN * bar:
            bad.append((k, e, e_ref[k]))
    print(f"{what}: worst ratio {worst:.2f} (median E_ref {med:.2e})")
    assert not bad, bad
    return worst


# --------------------------------------------------------------------------------------------------- head into decoder
# The VQ head 64 -> cfg.semantic_dim (K = cfg.codebook_size, the four-module proj) feeding the decoder of train_util case G4 through
# sem_features: loss = mse + 0.1 vq_loss as train.py's phase 1 forms it, one backward.  E2E_FEATURE_SEED: searched like FEATURE_SEED.
E2E_IN_DIM, E2E_WEIGHT_SEED, E2E_FEATURE_SEED, E2E_LOSS_W = 64, 6, 100, 0.1


@functools.lru_cache(maxsize=None)
def e2e_case(feature_seed=None):
    """(cfg, decoder state dict, decoder inputs, proj state dict, quantizer state dict, features [B, S, 64])"""
    import train_util as TU
    cfg, sd, inp = TU.case("G4")
    B, S = inp["f"].shape[0], inp["f"].shape[1]
    proj_sd, q_sd = synth_semantic_head(E2E_IN_DIM, cfg.semantic_dim, None, codebook_size=cfg.codebook_size, seed=E2E_WEIGHT_SEED)
    q_sd = dict(q_sd)
    q_sd["ema_cluster_size"], q_sd["ema_w"] = start_buffers(cfg.codebook_size, cfg.semantic_dim, q_sd["codebook.weight"], E2E_WEIGHT_SEED)
    h = synth_hubert_features(B, S, E2E_IN_DIM, E2E_FEATURE_SEED if feature_seed is None else feature_seed)
    return cfg, sd, inp, proj_sd, q_sd, h


def _e2e(dtype, feature_seed=None):
    import train_util as TU
    from oracle import edtts_oracle as O
    cfg, sd, inp, proj_sd, q_sd, h = e2e_case(feature_seed)
    head = Head(weights_of(proj_sd, q_sd), q_sd, dtype, commit=cfg.vq_commit)
    prm = {k: (v.to(dtype).clone().requires_grad_(k not in TU.BUFFERS) if v.is_floating_point() else v) for k, v in sd.items()}
    x = inp["x"].to(dtype).clone().requires_grad_(True)
    B, S = h.shape[0], h.shape[1]
    z = proj_forward(head.p, h.to(dtype).reshape(B * S, -1))
    zq, idx, vq_loss = head.quantize(z)
    out = O.decoder_forward(prm, x, inp["t"], None, inp["si"], zq.reshape(B, S, -1), heads=cfg.heads, window=cfg.attn_window_size)
    (((out - inp["target"].to(dtype)) ** 2).mean() + E2E_LOSS_W * vq_loss).backward()
    g = {k: v.grad for k, v in prm.items() if v.is_floating_point() and k not in TU.BUFFERS}
    g["d_x"] = x.grad
    g.update({"head." + k: v.grad for k, v in head.p.items()})
    return g, idx, head.last["gap"], vq_loss.detach()


@functools.lru_cache(maxsize=None)
def e2e_oracle(feature_seed=None):
    """(fp64 gradients -- decoder parameters by name, "d_x", "head.<canonical name>" --, E_ref, median E_ref, fp64 idx, fp32 idx, fp64 gap
    per frame, fp64 vq_loss)"""
    g64, idx64, gap, loss64 = _e2e(torch.float64, feature_seed)
    g32, idx32, _, _ = _e2e(torch.float32, feature_seed)
    e_ref = {k: rel_err(g32[k], g64[k]) for k in g64 if g64[k] is not None}
    return g64, e_ref, float(torch.tensor(sorted(e_ref.values())).median()), idx64, idx32, gap, loss64
