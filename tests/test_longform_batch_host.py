"""Batched long-form synthesis, host side: the new C symbols, the validation of InpaintSampler.generate_long_batch and of the new
in-painting keywords, and the per-utterance chunk plan.  No GPU needed."""
import os
import re

import pytest
import torch

from edge_diffusion_tts_amd import CFG, EdgeDiffusionDecoder, InpaintSampler, native
from edge_diffusion_tts_amd.schedule import DiffusionSchedule

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sampler():
    cfg = CFG(device="cpu")
    return InpaintSampler(cfg, DiffusionSchedule(cfg.diff_steps), EdgeDiffusionDecoder(cfg)), cfg


def utterances(cfg, rows=(80, 50, 128)):
    g = torch.Generator().manual_seed(0)
    return [torch.randn(1, r, cfg.semantic_dim, generator=g) for r in rows]


def test_header_declares_the_new_entry_points():
    header = open(os.path.join(REPO, "include", "edtts.h")).read()
    # the plain in-painting entry point keeps its signature: 21 parameters, the _len twin three more
    def n_params(name):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", header)
        return len(m.group(1).split(","))
    assert n_params("edtts_sample_inpaint") == 21
    assert n_params("edtts_sample_inpaint_len") == 24


def plan_args(cfg, smp, rows, totals, chunk=48, ov=12, hop=160, sr=8000):
    feats = utterances(cfg, rows)
    stats = []
    for t in totals:
        n = smp.chunk_plan(t, chunk, ov, hop)[0]
        stats.append([(0.0, 1.0)] * n)
    return feats, stats


def test_generate_long_batch_rejects_mismatched_lists():
    smp, cfg = sampler()
    feats, stats = plan_args(cfg, smp, (80, 50, 128), (100, 60, 150))
    with pytest.raises(ValueError, match="total_frames"):
        smp.generate_long_batch(feats, [100, 60], 48, 12, stats, seeds=[1, 2, 3], hop_length=160, sample_rate=8000)
    with pytest.raises(ValueError, match="chunk_stats"):
        smp.generate_long_batch(feats, [100, 60, 150], 48, 12, stats[:2], seeds=[1, 2, 3], hop_length=160, sample_rate=8000)
    with pytest.raises(ValueError, match="seeds"):  # too few seeds
        smp.generate_long_batch(feats, [100, 60, 150], 48, 12, stats, seeds=[1, 2], hop_length=160, sample_rate=8000)
    with pytest.raises(ValueError, match="latent_slices"):
        smp.generate_long_batch(feats, [100, 60, 150], 48, 12, stats, seeds=[1, 2, 3], latent_slices=[None], hop_length=160,
                                sample_rate=8000)
    with pytest.raises(ValueError, match="draws"):
        smp.generate_long_batch(feats, [100, 60, 150], 48, 12, stats, seeds=[1, 2, 3], draws=[None, None], hop_length=160,
                                sample_rate=8000)
    with pytest.raises(TypeError):  # seeds is keyword-only and required
        smp.generate_long_batch(feats, [100, 60, 150], 48, 12, stats)


def test_generate_long_batch_names_the_utterance():
    smp, cfg = sampler()
    feats, stats = plan_args(cfg, smp, (80, 50, 128), (100, 60, 150))
    bad = [stats[0], stats[1][:-1], stats[2]]
    with pytest.raises(ValueError, match=r"utterance 1: chunk_stats must hold \d+ \(mean, std\) pairs"):
        smp.generate_long_batch(feats, [100, 60, 150], 48, 12, bad, seeds=[1, 2, 3], hop_length=160, sample_rate=8000)
    with pytest.raises(ValueError, match="overlap_frames < chunk_frames"):
        smp.generate_long_batch(feats, [100, 60, 150], 48, 48, stats, seeds=[1, 2, 3], hop_length=160, sample_rate=8000)
    # a slice past the end of utterance 2's features is empty, as in generate_long
    short = utterances(cfg, (80, 50, 4))
    with pytest.raises(ValueError, match=r"utterance 2: chunk \d+: empty semantic slice"):
        smp.generate_long_batch(short, [100, 60, 150], 48, 12, stats, seeds=[1, 2, 3], hop_length=160, sample_rate=8000)


def test_generate_long_keeps_its_errors():
    smp, cfg = sampler()
    feats, stats = plan_args(cfg, smp, (80,), (100,))
    with pytest.raises(ValueError, match="overlap_frames < chunk_frames"):
        smp.generate_long(feats[0], 100, 48, 48, stats[0])
    with pytest.raises(ValueError, match="chunk_stats must hold"):
        smp.generate_long(feats[0], 100, 48, 12, stats[0][:-1], hop_length=160, sample_rate=8000)


@pytest.mark.parametrize("totals, rows", [((100, 60, 150, 48, 333), (80, 50, 128, 40, 300)), ((1000,), (1100,))])
def test_plan_matches_chunk_plan_and_latent_slices_per_utterance(totals, rows):
    smp, cfg = sampler()
    chunk, ov, hop, sr = 48, 12, 160, 8000
    feats, stats = plan_args(cfg, smp, rows, totals, chunk, ov, hop, sr)
    plans = smp.plan_long_batch(rows, totals, chunk, ov, stats, list(range(len(rows))), hop_length=hop, sample_rate=sr)
    for n, (t, r) in enumerate(zip(totals, rows)):
        n_chunks, c_samples, hop_samples = smp.chunk_plan(t, chunk, ov, hop)
        assert plans[n]["n_chunks"] == n_chunks
        want = smp.latent_slices(n_chunks, hop_samples, c_samples, sr)
        for (a, b), (l0, l1) in zip(plans[n]["slices"], want):
            assert feats[n][:, a:b].shape[1] == feats[n][:, l0:l1].shape[1] > 0
            assert torch.equal(feats[n][:, a:b], feats[n][:, l0:l1])


def test_plan_takes_per_utterance_total_samples_and_slices():
    smp, cfg = sampler()
    rows, totals = (128, 128), (100, 100)
    feats, stats = plan_args(cfg, smp, rows, totals)
    n0 = smp.chunk_plan(100, 48, 12, 160, total_samples=16000)[0]
    stats[0] = [(0.0, 1.0)] * n0
    custom = [(0, 10), (5, 20), (30, 31)]
    stats[1] = [(0.0, 1.0)] * 3
    plans = smp.plan_long_batch(rows, totals, 48, 12, stats, [0, 1], latent_slices=[None, custom], hop_length=160, sample_rate=8000,
                                total_samples=[16000, None])
    assert plans[0]["n_chunks"] == n0
    assert plans[1]["slices"] == custom


def test_inpaint_keywords_are_validated_before_any_device_work():
    smp, cfg = sampler()
    x = torch.zeros(2, 48, cfg.n_mels)
    f = torch.zeros(2, 20, cfg.semantic_dim)
    known = torch.zeros(2, 12, cfg.n_mels)
    with pytest.raises(ValueError, match="x_lengths"):
        smp.inpaint_teacher_refine(x, f, known, 12, 0.5, 2, noise=x, x_lengths=torch.tensor([48, 49]))
    with pytest.raises(ValueError, match="sem_lengths"):
        smp.inpaint_teacher_refine(x, f, known, 12, 0.5, 2, noise=x, sem_lengths=torch.tensor([0, 20]))
    with pytest.raises(ValueError, match="overlap_len = 12"):  # the call on row 1 alone would refuse this overlap
        smp.inpaint_teacher_refine(x, f, known, 12, 0.5, 2, noise=x, x_lengths=torch.tensor([48, 11]))
    with pytest.raises(ValueError, match="seeds"):
        smp.inpaint_student_sample((2, 48, cfg.n_mels), f, x_init=x, seeds=[1])
    with pytest.raises(TypeError):  # keyword-only
        smp.inpaint_teacher_refine(x, f, known, 12, 0.5, 2, 1.0, None, None, 0, torch.tensor([48, 48]))


def test_seed_tensor_keeps_the_bits():
    s = native.seed_tensor([0, 1, 2 ** 63, 2 ** 64 - 1, -1], 5, "cpu")
    assert s.dtype == torch.int64
    assert [v & 0xFFFFFFFFFFFFFFFF for v in s.tolist()] == [0, 1, 2 ** 63, 2 ** 64 - 1, 2 ** 64 - 1]
    with pytest.raises(ValueError, match="seeds"):
        native.seed_tensor([1, 2], 3, "cpu")
    with pytest.raises(ValueError, match="seeds"):
        native.seed_tensor(torch.zeros(3, dtype=torch.int32), 3, "cpu")
