"""Per-utterance lengths (ragged batches), host side: validation of the new keywords, unchanged size queries, the new C symbols
and the per-rank slicing of ShardedEdgeInference.  No GPU needed."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from edge_diffusion_tts_amd import CFG, EdgeDiffusionDecoder, native
from edge_diffusion_tts_amd.parallel import ShardedEdgeInference
from edge_diffusion_tts_amd.schedule import DiffusionSchedule, DPMSolverPP

LEN_SYMBOLS = ("edtts_decoder_forward_len", "edtts_generate_len", "edtts_sample_ddpm_len", "edtts_sample_multistep_len")


def dec():
    return EdgeDiffusionDecoder(CFG(device="cpu"))


@pytest.mark.parametrize("bad, err", [
    (torch.tensor([3, 4], dtype=torch.int32), "dtype torch.int64"),
    (torch.tensor([3.0, 4.0]), "dtype torch.int64"),
    (torch.tensor([[3, 4]]), r"shape \[2\]"),
    (torch.tensor([3, 4, 5]), r"shape \[2\]"),
    (torch.tensor([0, 4]), r"in \[1, 16\]"),
    (torch.tensor([3, 17]), r"in \[1, 16\]"),
    ([3, 4], "int64 tensor"),
])
def test_lengths_are_validated(bad, err):
    with pytest.raises(ValueError, match=err):
        native.lengths(bad, 2, 16, "cpu", "x_lengths")


def test_valid_cpu_lengths_pass_and_none_is_none():
    n = torch.tensor([1, 16])
    assert torch.equal(native.lengths(n, 2, 16, "cpu", "x_lengths"), n)
    assert native.lengths(None, 2, 16, "cpu", "x_lengths") is None


def test_forward_checks_its_length_keywords_first():
    d = dec()
    x, t, sem = torch.zeros(2, 32, 80), torch.zeros(2, dtype=torch.int64), torch.zeros(2, 16, dtype=torch.int64)
    with pytest.raises(ValueError, match="x_lengths"):
        d(x, t, sem, x_lengths=torch.tensor([33, 2]))
    with pytest.raises(ValueError, match="sem_lengths"):
        d(x, t, sem, sem_lengths=torch.tensor([1, 17]))
    with pytest.raises(ValueError, match="sem_lengths"):
        d(x, t, sem, sem_lengths=torch.tensor([1], dtype=torch.int64))
    with pytest.raises(TypeError):  # keyword-only
        d(x, t, sem, None, None, torch.tensor([1, 2]))


def test_dpm_solver_checks_its_length_keywords_first():
    d = dec()
    with pytest.raises(ValueError, match="x_lengths"):
        DPMSolverPP(DiffusionSchedule(1000)).sample(d, torch.zeros(2, 32, 80), None, 4,
                                                    sem_idx=torch.zeros(2, 16, dtype=torch.int64),
                                                    x_lengths=torch.tensor([0, 2]))


def test_sizes_do_not_depend_on_lengths():
    """A workspace sized for (B, T, S) serves every ragged call up to that shape: no query takes lengths, and the library's sizes are
    those of the parent's formula (a regression pin against a length-dependent workspace)."""
    d = dec()
    ws = native.workspace_bytes(d.dims(), 4, 64, 32, 4)
    assert ws == native.workspace_bytes(d.dims(), 4, 64, 32, 4) > 0
    assert native.packed_bytes(d.dims()) > 0
    for fn in (native.workspace_bytes, native.packed_bytes):
        assert "len" not in fn.__code__.co_varnames


def test_len_symbols_are_declared_exported_and_bound():
    for sym in LEN_SYMBOLS:
        assert hasattr(native.lib(), sym)


def _stub_len(sem, num_steps, x, lens):
    """A stand-in local sampler: row b = its length, so the gathered result shows which lengths each rank received."""
    return x * 0 + lens.to(x.dtype)[:, None, None] + 1000 * sem[:, :1, None].to(x.dtype)


def _stub3(sem, num_steps, x):
    return x * 2 + sem.sum(1).to(x.dtype)[:, None, None]


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        total, S, m = 6, 4, 3
        sem = torch.arange(total, dtype=torch.int64)[:, None].repeat(1, S)
        lens = torch.tensor([1, 4, 2, 3, 4, 1], dtype=torch.int64)
        x = torch.zeros(total, 2 * S, m)
        out = ShardedEdgeInference(local_generate=_stub_len).generate_mel(sem, 4, x_T=x, sem_lengths=lens)
        ref = _stub_len(sem, 4, x, lens)
        ok = torch.equal(out, ref)
        # micro-batches: successive slices of the rank's rows take successive lengths
        out_mb = ShardedEdgeInference(local_generate=_stub_len, micro_batches=3 if world == 2 else 1).generate_mel(
            sem, 4, x_T=x, sem_lengths=lens)
        ok = ok and torch.equal(out_mb, ref)
        # without lengths the local sampler is called with three arguments, as before
        out3 = ShardedEdgeInference(local_generate=_stub3).generate_mel(sem, 4, x_T=x + 1)
        ok = ok and torch.equal(out3, _stub3(sem, 4, x + 1))
        q.put((rank, ok))
    except Exception as e:  # noqa: BLE001 -- reported to the parent
        q.put((rank, repr(e)))
    finally:
        dist.destroy_process_group()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("world", [1, 2])
def test_sharded_generate_slices_lengths_per_rank(world):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(60)
    assert res == {r: True for r in range(world)}


def test_sharded_generate_validates_lengths():
    sh = ShardedEdgeInference(local_generate=_stub_len)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        with pytest.raises(ValueError, match="sem_lengths"):
            sh.generate_mel(torch.zeros(2, 4, dtype=torch.int64), 4, x_T=torch.zeros(2, 8, 3), sem_lengths=torch.tensor([1.0, 2.0]))
    finally:
        dist.destroy_process_group()
