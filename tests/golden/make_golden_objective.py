#!/usr/bin/env python3
"""Training-objective fixture for tests/golden: made by running the REFERENCE on CPU (build container only).

    python tests/golden/make_golden_objective.py

objective   the reference's own normalize_mel (utils/audio.py), DiffusionSchedule.q_sample / get_v_target / predict_x0_from_v
            (schedule.py), F.mse_loss and F.cosine_similarity as train_v2.py:135-154 calls them, and
            ConsistencyTrainer.progressive_distillation_loss (without and with a teacher) and consistency_loss
            (training/consistency.py:60-122), at B x T x M = 3 x 24 x 20 in fp32.  Fixed inputs; the reference draws its noise with
            torch.randn_like and its timesteps with torch.randint, so both are replaced for the duration of a call by functions that
            hand out the recorded tensors (t of the distillation stage: get_timestep_pairs' own arithmetic on the recorded step
            indices).  The decoders are stubs that return a recorded prediction and check the x_t they are given.
            Every quantity is also computed by the same functions on fp64 inputs (the schedule's tables stay the reference's fp32
            ones, upcast); "tol.<name>" is max|fp32 - fp64|: the reference's own fp32-against-fp64 difference, the tolerance of
            tests/test_objective_host.py.  Inputs + outputs only.
"""
import os
import sys
from unittest import mock

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402,F401  (sets sys.path for the reference, chdirs to a scratch dir)
from make_golden import OUT  # noqa: E402
import edge_diffusion_tts as ref  # noqa: E402
from edge_diffusion_tts.training.consistency import ConsistencyTrainer  # noqa: E402
from edge_diffusion_tts.utils.audio import normalize_mel  # noqa: E402

B, T, M, NUM_STEPS = 3, 24, 20, 50
STEP_IDX = (0, 49, 17)          # -> t = (19, 999, 359) with diff_steps = 1000, stride 20
T1, T2 = (1, 999, 420), (999, 1, 77)


class Stub(torch.nn.Module):
    """A decoder that returns a recorded prediction and keeps what it was called with."""

    def __init__(self, preds):
        super().__init__()
        self.preds, self.calls = list(preds), []

    def forward(self, x_t, t, sem_idx, step_idx):
        self.calls.append((x_t.detach().clone(), t.clone()))
        return self.preds[len(self.calls) - 1]


def run(dtype, inp):
    """Every recorded quantity from the reference's functions on inputs of `dtype`."""
    cfg = ref.CFG(device="cpu")
    sch = ref.DiffusionSchedule(cfg.diff_steps)
    mel, noise = inp["mel"].to(dtype), inp["noise"].to(dtype)
    out = {}
    # ---- train_v2.py:112-154 with its own helpers
    mel_n, mean, std = normalize_mel(mel)
    t = torch.tensor(T1)
    x_t, _ = sch.q_sample(mel_n, t, noise)
    v_pred = inp["pred"].to(dtype)
    v_target = sch.get_v_target(mel_n, noise, t)
    x0 = sch.predict_x0_from_v(x_t, t, v_pred)
    out.update(mean=mean, std=std, mel_n=mel_n, x_t=x_t, v_target=v_target, x0=x0, loss_v=F.mse_loss(v_pred, v_target),
               loss_eps=F.mse_loss(v_pred, noise), x0_mse=F.mse_loss(x0, mel_n),
               x0_cos=F.cosine_similarity(x0.flatten(1), mel_n.flatten(1), dim=1).mean())
    # ---- training/consistency.py with stub decoders; randn_like / randint hand out the recorded draws
    draws = []
    fake_randn = lambda x: noise.to(x.dtype)
    fake_randint = lambda *a, **k: draws.pop(0)
    with mock.patch.object(torch, "randn_like", fake_randn), mock.patch.object(torch, "randint", fake_randint):
        student, teacher = Stub([inp["pred"]] * 2), Stub([inp["teacher_pred"]])
        tr = ConsistencyTrainer(cfg, sch, None, student)
        draws[:] = [torch.tensor(STEP_IDX)]
        loss, x0_s, _ = tr.progressive_distillation_loss(mel, None, NUM_STEPS)       # no teacher: the v-prediction loss
        out.update(distill_t=student.calls[0][1], loss_distill_v=loss, distill_x_t=student.calls[0][0])
        tr.teacher = teacher
        draws[:] = [torch.tensor(STEP_IDX)]
        loss, x0_s, _ = tr.progressive_distillation_loss(mel, None, NUM_STEPS)
        out.update(loss_distill=loss, distill_x0=x0_s)
        two = Stub([inp["pred"], inp["pred2"]])
        tr = ConsistencyTrainer(cfg, sch, None, two)
        draws[:] = [torch.tensor(T1), torch.tensor(T2)]
        loss, x0_1, _ = tr.consistency_loss(mel, None)
        out.update(loss_consistency=loss, consistency_x0=x0_1)
        assert torch.equal(two.calls[0][1], torch.tensor(T1)) and torch.equal(two.calls[1][1], torch.tensor(T2))
        assert not draws
    return {k: v.detach() for k, v in out.items()}


def main():
    g = torch.Generator().manual_seed(2025)
    inp = dict(mel=torch.randn(B, T, M, generator=g) * 1.5 - 4.0, noise=torch.randn(B, T, M, generator=g),
               pred=torch.randn(B, T, M, generator=g), teacher_pred=torch.randn(B, T, M, generator=g),
               pred2=torch.randn(B, T, M, generator=g))
    o32, o64 = run(torch.float32, inp), run(torch.float64, inp)
    assert torch.equal(o32["distill_t"], o64["distill_t"])
    out = {"dims": np.array([B, T, M, NUM_STEPS], np.int64), "t1": np.array(T1, np.int64), "t2": np.array(T2, np.int64)}
    out.update({"in." + k: v.numpy() for k, v in inp.items()})
    for k, v in o32.items():
        out[k] = v.numpy()
        if v.is_floating_point():
            assert v.dtype == torch.float32, (k, v.dtype)
            out["tol." + k] = np.float64((v.double() - o64[k].double()).abs().max())
    print("objective: " + ", ".join(f"{k} {float(out[k]):.6f} (tol {out['tol.' + k]:.1e})" for k in o32 if k.startswith(("loss", "x0_m", "x0_c"))))
    np.savez_compressed(os.path.join(OUT, "objective.npz"), **out)
    print(f"objective.npz: {os.path.getsize(os.path.join(OUT, 'objective.npz'))} bytes")


if __name__ == "__main__":
    main()
