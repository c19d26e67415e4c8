"""Shared by test_inpaint_mask_host.py and test_inpaint_mask_gpu.py: the shapes, the masks, and the in-painting
samplers with a per-frame mask composed from the oracle's public functions on the CPU -- the reference's rule `x[known] = q_sample(
known_mel, t_i)` before every step and `x[known] = known_mel` after the last, with the mask anywhere instead of a prefix."""
import torch

from oracle import edtts_oracle as O

B, T, S = 3, 41, 20
N_STUDENT, STEPS, STRENGTH = 4, 5, 0.5
T_LEN, S_LEN, SEEDS = [41, 33, 12], [20, 16, 5], [5, 2 ** 40 + 1, 77]
# Kept frames per row, half-open.  Row 0: frame 0, the last frame (40), one isolated kept frame (10) and one isolated free frame (25).
# Row 1: a run that crosses t_len = 33 (its live part ends in the last live frame, 32).  Row 2: an isolated kept frame and a run that
# crosses t_len = 12.  Every row keeps 20 % .. 80 % of its frames, counted over T and over its live frames.
KEEP = [[(0, 6), (10, 11), (20, 25), (26, 30), (40, 41)],
        [(5, 15), (30, 37)],
        [(3, 4), (6, 9), (10, 20)]]

CONFIGS = {
    "32/2/80": (dict(hidden=32, heads=2), {}),
    "160/4/80": ({}, {}),
    "generic 50/5/45": (dict(hidden=50, heads=5, n_mels=45, semantic_dim=7, layers=2), dict(kernels="generic")),
    "bf16 64/2/80": (dict(hidden=64, heads=2), dict(compute_dtype="bf16")),
}
FP32 = [n for n in CONFIGS if not n.startswith("bf16")]


def keep_mask():
    m = torch.zeros(B, T, dtype=torch.bool)
    for b, row in enumerate(KEEP):
        for lo, hi in row:
            m[b, lo:hi] = True
    return m


def inputs(cfg, seed=3):
    """CPU tensors of one case: the start points, the context, a whole known mel and per-step noise for it."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(x_init=r(B, T, cfg.n_mels), x_coarse=r(B, T, cfg.n_mels).clamp(-3, 3), sem=r(B, S, cfg.semantic_dim),
                known=r(B, T, cfg.n_mels).clamp(-3, 3), noise=r(B, T, cfg.n_mels), noise_k=r(STEPS, B, T, cfg.n_mels))


def _blend(x, keep, sab, s1m, known, nz):
    x = x.clone()
    x[keep] = (sab * known + s1m * nz)[keep]
    return x


def _v(sd, cfg, x, t, step_idx, sem, scale):
    n = x.shape[0]
    tt, si = torch.full((n,), t, dtype=torch.long), torch.full((n,), step_idx, dtype=torch.long)
    kw = dict(heads=cfg.heads, window=cfg.attn_window_size)
    v = O.decoder_forward(sd, x, tt, None, si, sem, **kw)
    if scale != 1.0:
        vu = O.decoder_forward(sd, x, tt, None, si, torch.zeros_like(sem), **kw)
        v = vu + scale * (v - vu)
    return v


def oracle_first_order(sd, cfg, x, sem, times, step_idx, known, keep, noise_k, scale=1.0):
    """The loop of the oracle's inpaint_loop, statement for statement, with `[keep]` where it has `[:, :overlap_len]`."""
    tabs = O.schedule_tables(cfg.diff_steps)
    sab, s1m, ab = tabs["sqrt_alpha_bar"], tabs["sqrt_one_minus_alpha_bar"], tabs["alpha_bar"]
    x = x.clone()
    for i, t in enumerate(times):
        t_next = times[i + 1] if i < len(times) - 1 else 0
        x = _blend(x, keep, sab[t], s1m[t], known, noise_k[i])
        v = _v(sd, cfg, x, t, step_idx, sem, scale)
        x0 = torch.clamp(sab[t] * x - s1m[t] * v, -3, 3)
        eps = s1m[t] * x + sab[t] * v
        x = torch.sqrt(ab[t_next]) * x0 + torch.sqrt(1 - ab[t_next]) * eps
    x[keep] = known[keep]
    return x


def oracle_student(sd, cfg, d, keep, rows=slice(None), frames=T):
    c = lambda k: d[k][rows, :frames]
    return oracle_first_order(sd, cfg, c("x_init"), d["sem"][rows], O.linspace_times(cfg.diff_steps - 1, N_STUDENT), 3, c("known"),
                              keep[rows, :frames], d["noise_k"][:N_STUDENT, rows, :frames])


def oracle_teacher(sd, cfg, d, keep, scale, rows=slice(None), frames=T):
    tabs = O.schedule_tables(cfg.diff_steps)
    c = lambda k: d[k][rows, :frames]
    t_start = int(cfg.diff_steps * STRENGTH)
    x = tabs["sqrt_alpha_bar"][t_start] * c("x_coarse") + tabs["sqrt_one_minus_alpha_bar"][t_start] * c("noise")
    return oracle_first_order(sd, cfg, x, d["sem"][rows], O.linspace_times(t_start, STEPS), 0, c("known"), keep[rows, :frames],
                              d["noise_k"][:, rows, :frames], scale)


def oracle_dpm(sd, cfg, d, keep, order, scale, rows=slice(None), frames=T, sem_rows=S):
    """inpaint_dpm_refine under a mask: the start point of the oracle's inpaint_teacher_refine, the times of dpmpp_timesteps, the x0 and
    update expressions as dpmpp_sample has them, the blend before every step and the force after the last at `[keep]`."""
    tabs = O.schedule_tables(cfg.diff_steps)
    a_t, s_t, lam = tabs["sqrt_alpha_bar"], tabs["sqrt_one_minus_alpha_bar"], tabs["lambda_t"]
    c = lambda k: d[k][rows, :frames]
    known, keep, sem = c("known"), keep[rows, :frames], d["sem"][rows, :sem_rows]
    t_start = int(cfg.diff_steps * STRENGTH)
    ts = O.dpmpp_timesteps(lam, STEPS, t_start)
    x = a_t[t_start] * c("x_coarse") + s_t[t_start] * c("noise")
    x0_hist, t_hist = [], []
    for i, t in enumerate(ts):
        x = _blend(x, keep, a_t[t], s_t[t], known, d["noise_k"][i, rows, :frames])
        v = _v(sd, cfg, x, t, 0, sem, scale)
        x0 = torch.clamp(a_t[t] * x - s_t[t] * v, -3, 3)
        tp = ts[i + 1] if i < len(ts) - 1 else 0
        h = lam[tp] - lam[t]
        if order == 1 or len(x0_hist) == 0:
            x = (s_t[tp] / s_t[t]) * x + a_t[tp] * (1 - torch.exp(-h)) * x0
        elif order == 2 or len(x0_hist) == 1:
            r = (lam[t_hist[-1]] - lam[tp]) / h
            d1 = (1 / r) * (x0 - x0_hist[-1])
            x = (s_t[tp] / s_t[t]) * x + a_t[tp] * (1 - torch.exp(-h)) * x0 + a_t[tp] * ((1 - torch.exp(-h)) / h + 1) * d1 * 0.5
        else:
            p = [x0] + x0_hist[-2:]
            d1 = p[0] - p[1]
            d2 = p[0] - 2 * p[1] + p[2]
            x = ((s_t[tp] / s_t[t]) * x + a_t[tp] * (1 - torch.exp(-h)) * p[0] + a_t[tp] * ((1 - torch.exp(-h)) / h + 1) * d1 * 0.5
                 + a_t[tp] * ((1 - torch.exp(-h)) / (h ** 2) + 0.5 / h + 0.5) * d2 / 6)
        x0_hist, t_hist = (x0_hist + [x0])[-2:], (t_hist + [tp])[-2:]
    x[keep] = known[keep]
    return x
