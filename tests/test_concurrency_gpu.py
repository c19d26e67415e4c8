"""Several streams and threads on one decoder: every sampler and the forward, called from up to four torch streams (one thread or
several) without synchronising in between, give bitwise the results of the same calls made one after another
(include/edtts.h "threads and streams"; decoder.workspace: one workspace per stream and shape).
Run on the GPU box: python -m pytest tests -m gpu."""
import threading

import pytest
import torch

from edge_diffusion_tts_amd import (CFG, DiffusionSchedule, DPMSolverPP, EdgeDiffusionDecoder, EdgeInference, InpaintSampler,
                                    native, synth_state_dict)

pytestmark = pytest.mark.gpu
DEV = "cuda"


def make_decoder(cfg, seed=0, **kw):
    dec = EdgeDiffusionDecoder(cfg, **kw)
    dec.load_state_dict(synth_state_dict(cfg, seed, max_pos=dec.max_len, max_ctx_pos=dec.max_context_len))
    return dec.to(DEV).eval()


def make_infer(cfg, dec):
    return EdgeInference(cfg, DiffusionSchedule(cfg.diff_steps).to(DEV), torch.nn.Identity(), dec)


def token_inputs(n, B, S, seed, mels=80, codebook=512):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randint(0, codebook, (B, S), generator=g).to(DEV), torch.randn(B, 2 * S, mels, generator=g).to(DEV))
            for _ in range(n)]


def run_concurrently(calls, n_streams, rounds):
    """calls[r][i]() on stream i, rounds after one another, no synchronisation in between; returns outs[r][i]."""
    main = torch.cuda.current_stream()
    streams = [torch.cuda.Stream() for _ in range(n_streams)]
    for s in streams:
        s.wait_stream(main)  # (the inputs were made on the main stream)
    outs = [[None] * n_streams for _ in range(rounds)]
    for r in range(rounds):
        for i, s in enumerate(streams):
            with torch.cuda.stream(s):
                outs[r][i] = calls[r][i]()
    torch.cuda.synchronize()
    return outs


def test_two_streams_get_two_workspaces():
    cfg = CFG(device=DEV)
    dec = make_decoder(cfg)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        a = dec.workspace(4, 128, 64, 4, torch.device(DEV))
    with torch.cuda.stream(s2):
        b = dec.workspace(4, 128, 64, 4, torch.device(DEV))
    assert a.data_ptr() != b.data_ptr()
    with torch.cuda.stream(s1):
        assert dec.workspace(4, 128, 64, 4, torch.device(DEV)).data_ptr() == a.data_ptr()
    assert dec.workspace(4, 128, 64, 4, torch.device(DEV), stream=s2).data_ptr() == b.data_ptr()
    assert dec.workspace(4, 128, 64, 4, torch.device(DEV)).data_ptr() not in (a.data_ptr(), b.data_ptr())  # the default stream's
    torch.cuda.synchronize()
    assert not bool(a.any()) and not bool(b.any())


@pytest.mark.parametrize("n_streams", [2, 4])
def test_generate_mel_on_several_streams_is_bitwise_sequential(n_streams):
    """B = 256, T = 512 (the default setting cuts each call into two sub-batches on side streams of its own), different inputs on
    every stream, three rounds without a sync."""
    cfg = CFG(device=DEV)
    infer = make_infer(cfg, make_decoder(cfg))
    rounds, B, S = 3, 256, 256
    inputs = token_inputs(rounds * n_streams, B, S, seed=n_streams)
    alone = [infer.generate_mel(sem, 4, x_T=x) for sem, x in inputs]
    torch.cuda.synchronize()
    calls = [[(lambda sem=sem, x=x: infer.generate_mel(sem, 4, x_T=x)) for sem, x in inputs[r * n_streams:(r + 1) * n_streams]]
             for r in range(rounds)]
    outs = run_concurrently(calls, n_streams, rounds)
    for r in range(rounds):
        for i in range(n_streams):
            assert torch.equal(outs[r][i], alone[r * n_streams + i]), (r, i)


def test_generate_mel_on_two_threads_is_bitwise_sequential():
    cfg = CFG(device=DEV)
    infer = make_infer(cfg, make_decoder(cfg))
    rounds, B, S = 3, 256, 256
    inputs = token_inputs(2 * rounds, B, S, seed=5)
    alone = [infer.generate_mel(sem, 4, x_T=x) for sem, x in inputs]
    torch.cuda.synchronize()
    outs, errors = {}, []

    def worker(t):
        try:
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.default_stream())
            with torch.cuda.stream(s):
                for r in range(rounds):
                    sem, x = inputs[2 * r + t]
                    outs[(r, t)] = infer.generate_mel(sem, 4, x_T=x)
            s.synchronize()
        except Exception as e:  # (surfaced below: an exception in a thread does not fail the test by itself)
            errors.append(repr(e))

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=300)
    assert not errors, errors
    for r in range(rounds):
        for t in range(2):
            assert torch.equal(outs[(r, t)], alone[2 * r + t]), (r, t)


def test_other_samplers_on_several_streams():
    """sample_ddpm (in-kernel Philox noise), DPM-Solver++ order 2 on features, guided in-painting (two workspaces per call) and
    the forward, on three streams at once."""
    cfg = CFG(device=DEV)
    dec = make_decoder(cfg)
    infer = make_infer(cfg, dec)
    sch = DiffusionSchedule(cfg.diff_steps).to(DEV)
    solver = DPMSolverPP(sch, order=2)
    smp = InpaintSampler(cfg, sch, dec)
    n, rounds, B, S = 3, 2, 32, 128
    g = torch.Generator().manual_seed(7)
    toks = token_inputs(n * rounds, B, S, seed=8)
    feats = [torch.randn(B, S, cfg.semantic_dim, generator=g).to(DEV) for _ in range(n * rounds)]
    known = [torch.randn(B, 24, 80, generator=g).to(DEV) for _ in range(n * rounds)]
    t = torch.full((B,), 500, device=DEV)

    def jobs(k):
        sem, x = toks[k]
        return [lambda: infer.sample_ddpm(sem, 6, x_T=x, seed=k),
                lambda: solver.sample(dec, x, feats[k], num_steps=4),
                lambda: smp.inpaint_teacher_refine(x, feats[k], known[k], 24, strength=0.3, steps=3, cfg_scale=2.5, seed=k),
                lambda: dec(x, t, sem, None)]

    alone = [[job() for job in jobs(k)] for k in range(n * rounds)]
    torch.cuda.synchronize()
    calls = [[(lambda k=r * n + i: [job() for job in jobs(k)]) for i in range(n)] for r in range(rounds)]
    outs = run_concurrently(calls, n, rounds)
    for r in range(rounds):
        for i in range(n):
            for j, (o, a) in enumerate(zip(outs[r][i], alone[r * n + i])):
                assert torch.equal(o, a), (r, i, ("ddpm", "dpm++", "inpaint", "forward")[j])


def test_generic_kernels_on_several_streams():
    cfg = CFG(device=DEV, hidden=224, heads=7)
    infer = make_infer(cfg, make_decoder(cfg, kernels="generic"))
    n, rounds, B, S = 3, 2, 6, 45
    inputs = token_inputs(n * rounds, B, S, seed=9, codebook=cfg.codebook_size)
    alone = [infer.generate_mel(sem, 4, x_T=x) for sem, x in inputs]
    torch.cuda.synchronize()
    calls = [[(lambda sem=sem, x=x: infer.generate_mel(sem, 4, x_T=x)) for sem, x in inputs[r * n:(r + 1) * n]] for r in range(rounds)]
    outs = run_concurrently(calls, n, rounds)
    for r in range(rounds):
        for i in range(n):
            assert torch.equal(outs[r][i], alone[r * n + i]), (r, i)


def test_sub_batches_on_two_caller_streams_in_one_thread():
    """set_substreams(4) and B = 512, T = 512: every call forks three side streams; the two caller streams of one thread get
    side streams of their own and join only their own branches."""
    cfg = CFG(device=DEV)
    dec = make_decoder(cfg)
    infer = make_infer(cfg, dec)
    B, S = 512, 256
    prev = native.set_substreams(4)
    try:
        assert native.substreams_for(dec.dims(), B, 2 * S) == 4
        inputs = token_inputs(4, B, S, seed=10)
        alone = [infer.generate_mel(sem, 2, x_T=x) for sem, x in inputs]
        torch.cuda.synchronize()
        calls = [[(lambda sem=sem, x=x: infer.generate_mel(sem, 2, x_T=x)) for sem, x in inputs[r * 2:(r + 1) * 2]] for r in range(2)]
        outs = run_concurrently(calls, 2, 2)
        for r in range(2):
            for i in range(2):
                assert torch.equal(outs[r][i], alone[2 * r + i]), (r, i)
    finally:
        native.set_substreams(prev)


def test_graphs_captured_on_two_streams_replay_concurrently():
    cfg = CFG(device=DEV)
    dec = make_decoder(cfg)
    infer = make_infer(cfg, dec)
    B, S = 32, 256
    (sem1, x1), (sem2, x2) = token_inputs(2, B, S, seed=11)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    graphs = [torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()]
    eager, static_out = [], []
    for s, (sem, x) in zip(streams, ((sem1, x1), (sem2, x2))):
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):  # warm-up on the stream the graph is captured on: the capture takes its workspace
            eager.append(infer.generate_mel(sem, 4, x_T=x))
    torch.cuda.synchronize()
    for s, gr, (sem, x) in zip(streams, graphs, ((sem1, x1), (sem2, x2))):
        with torch.cuda.graph(gr, stream=s):
            static_out.append(infer.generate_mel(sem, 4, x_T=x))
    ws = [dec.workspace(B, 2 * S, S, 4, x1.device, stream=s) for s in streams]
    assert ws[0].data_ptr() != ws[1].data_ptr() and all(k[-1] in (s.cuda_stream for s in streams) for k in dec._pinned_workspaces)
    assert len(dec._pinned_workspaces) == 2
    for _ in range(3):
        static_out[0].zero_(); static_out[1].zero_()
        for s, gr in zip(streams, graphs):
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(static_out[0], eager[0]) and torch.equal(static_out[1], eager[1])
    del graphs, gr
    assert dec.release_pinned(B=B) == 2


def test_first_call_on_a_second_stream_waits_for_the_pack():
    """A fresh decoder: stream s1 is busy, then packs the weights (its first call); s2's first call, enqueued right behind on the
    host, must read the packed blob only after that pack."""
    cfg = CFG(device=DEV)
    ref = make_infer(cfg, make_decoder(cfg))
    (sem, x), = token_inputs(1, 8, 128, seed=12)
    expect = ref.generate_mel(sem, 4, x_T=x)
    infer = make_infer(cfg, make_decoder(cfg))
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        big = torch.randn(4096, 4096, device=DEV)
        for _ in range(20):  # (keeps s1 busy for a while: the pack behind it starts late)
            big = (big @ big).tanh_()
        out1 = infer.generate_mel(sem, 4, x_T=x)
    with torch.cuda.stream(s2):
        out2 = infer.generate_mel(sem, 4, x_T=x)
    torch.cuda.synchronize()
    assert torch.equal(out1, expect) and torch.equal(out2, expect)


def stale_blob_race(module, fresh, change, call):
    """The other modules' packed blobs are ordered across streams like the decoder's (_cache.PackedBlob).  The blob is packed from
    W1 by a warm call; one weight is changed in place (W2); stream s1 is kept busy and then makes the call, which re-packs behind
    the busy work; s2 makes the same call right away, and so do two more streams (streams that share a hardware queue run in
    submission order whether they wait or not, and a process here has four queues).  Without the wait for the pack they read a
    valid but stale blob (W1's), never unwritten memory.  Returns (s1's result, the other streams' results, the result of ``fresh``,
    a module loaded with W2)."""
    call(module)
    torch.cuda.synchronize()
    with torch.no_grad():
        change(module)
    torch.cuda.synchronize()
    fresh.load_state_dict(module.state_dict())
    expect = call(fresh)
    torch.cuda.synchronize()
    s1, others = torch.cuda.Stream(), [torch.cuda.Stream() for _ in range(3)]
    with torch.cuda.stream(s1):
        big = torch.randn(4096, 4096, device=DEV)
        for _ in range(20):  # (keeps s1 busy for a while: the re-pack behind it starts late)
            big = (big @ big).tanh_()
        out1 = call(module)
    outs = []
    for s in others:
        with torch.cuda.stream(s):
            outs.append(call(module))
    torch.cuda.synchronize()
    return out1, outs, expect


def test_hubert_call_on_a_second_stream_waits_for_the_repack():
    import json
    import os
    import numpy as np
    from edge_diffusion_tts_amd import NativeHubert
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hubert_small.npz"))  # (as test_hubert_gpu.small_model(3))
    sd = {k[2:]: torch.from_numpy(z[k].astype(np.float32)) for k in z.files if k.startswith("w:")}
    wav = torch.from_numpy(z["wav"].astype(np.float32)).to(DEV)

    def small_model():
        m = NativeHubert(json.loads(bytes(z["config"]).decode()), 3)
        m.load_state_dict(sd)
        return m.to(DEV).eval()

    def change(m):
        m._get("encoder.layer_norm.weight").mul_(1.5)
        m._get("feature_projection.projection.bias").add_(0.25)
    out1, outs, expect = stale_blob_race(small_model(), small_model(), change, lambda m: m(wav))
    assert torch.equal(out1, expect) and all(torch.equal(o, expect) for o in outs)


def semantic_head(quantizer, **kw):
    from edge_diffusion_tts_amd import SemanticEncoder
    from edge_diffusion_tts_amd.synth import synth_semantic_head
    cfg = CFG(device=DEV) if quantizer == "fsq" else CFG(device=DEV, use_fsq=False, codebook_size=64)
    proj_sd, q_sd = synth_semantic_head(64, cfg.semantic_dim, cfg.fsq_levels if quantizer == "fsq" else None, 64)
    enc = SemanticEncoder(cfg, in_dim=64, **kw)
    enc.proj.load_state_dict(proj_sd)
    enc.vq.load_state_dict(q_sd)
    return enc.to(DEV).eval()


def flip_last_linear(enc):
    enc.proj.final.weight.mul_(-1.0)
    enc.proj.final.bias.add_(0.25)


@pytest.mark.parametrize("quantizer", ["fsq", "vq"])
def test_quantize_features_on_a_second_stream_waits_for_the_repack(quantizer):
    from edge_diffusion_tts_amd.synth import synth_hubert_features
    h = synth_hubert_features(2, 50, 64, 3).to(DEV)
    out1, outs, (zq, idx, *_) = stale_blob_race(semantic_head(quantizer), semantic_head(quantizer), flip_last_linear,
                                                lambda m: m.quantize_features(h))
    for k, (zq_k, idx_k, *_) in enumerate([out1] + outs):
        assert torch.equal(idx_k, idx) and torch.equal(zq_k, zq), k


def test_semantic_training_step_on_a_second_stream_waits_for_the_repack():
    """autograd=True, FSQ: the forward and the backward read the inference blob and the training-only blob (_pack and _tpack)."""
    from edge_diffusion_tts_amd.synth import synth_hubert_features
    h = synth_hubert_features(2, 50, 64, 3).to(DEV)
    C = torch.randn(2, 50, 128, generator=torch.Generator().manual_seed(4)).to(DEV)

    def step(m):
        zq = m.quantize_features(h)[0]
        return (zq.detach(), *torch.autograd.grad((zq * C).sum(), m.get_trainable_params()))
    out1, outs, expect = stale_blob_race(semantic_head("fsq", autograd=True), semantic_head("fsq", autograd=True), flip_last_linear, step)
    assert len(expect) == 11 and all(bool(g.abs().sum() > 0) for g in expect)
    for k, out in enumerate([out1] + outs):
        for j, (a, e) in enumerate(zip(out, expect)):
            assert torch.equal(a, e), (k, j)


def test_index_errors_stay_with_their_stream():
    cfg = CFG(device=DEV)
    dec = make_decoder(cfg)
    infer = make_infer(cfg, dec)
    B, S = 4, 64
    (sem, x), = token_inputs(1, B, S, seed=13)
    bad = sem.clone()
    bad[1, 3] = 512
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for s in (s1, s2):
        s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s1):
        infer.generate_mel(bad, 4, x_T=x)
    with torch.cuda.stream(s2):
        infer.generate_mel(sem, 4, x_T=x)
    dev = x.device  # (the device the samplers key their workspaces by)
    with torch.cuda.stream(s2):
        assert native.index_errors(dec.workspace(B, 2 * S, S, 4, dev)) == 0
    with torch.cuda.stream(s1):
        assert native.index_errors(dec.workspace(B, 2 * S, S, 4, dev)) == 1
        assert native.index_errors(dec.workspace(B, 2 * S, S, 4, dev)) == 0
