"""DiffusionObjective without a GPU: the oracle of tests/objective_util.py against the fixture recorded from the reference
(tests/golden/objective.npz, tests/golden/make_golden_objective.py), the oracle's two forms against each other, and the argument
checks that come before any library call.  Run with: python -m pytest tests -m "not gpu"."""
import os

import numpy as np
import pytest
import torch

import objective_util as U
from edge_diffusion_tts_amd import DiffusionObjective, DiffusionSchedule, native
from edge_diffusion_tts_amd import objective as objective_module

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "objective.npz")


@pytest.fixture(scope="module")
def recorded():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _fixture_case(recorded, t, t2, pred2="pred2"):
    f = lambda k: torch.from_numpy(recorded["in." + k])
    return dict(mel=f("mel"), noise=f("noise"), pred=f("pred"), pred2=f(pred2), t=torch.from_numpy(np.asarray(t)),
                t2=torch.from_numpy(np.asarray(t2)))


def _close(got, recorded, name):
    err = float((got.detach().double() - torch.from_numpy(np.asarray(recorded[name])).double()).abs().max())
    tol = float(recorded["tol." + name])
    print(f"{name}: |oracle - reference| {err:.2e}, the reference's own fp32-against-fp64 difference {tol:.2e}")
    assert err <= tol, (name, err, tol)


def test_the_fp32_oracle_reproduces_the_reference(recorded):
    """Every recorded quantity, within the reference's own fp32-against-fp64 difference on this fixture (stored as tol.<name>)."""
    inp = _fixture_case(recorded, recorded["t1"], recorded["t2"])
    v = U.padded(inp, "v", torch.float32)
    for name, key in (("mean", "mean"), ("std", "std"), ("x_t", "x_t"), ("target", "v_target"), ("loss", "loss_v"), ("x0_mse", "x0_mse"),
                      ("x0_cos", "x0_cos")):
        _close(v[name], recorded, key)
    _close(U.padded(inp, "eps", torch.float32)["loss"], recorded, "loss_eps")
    _close(U.padded(inp, "consistency", torch.float32)["loss"], recorded, "loss_consistency")
    # the distillation stage ran at get_timestep_pairs' timesteps, the teacher's prediction in the place of pred2
    inp = _fixture_case(recorded, recorded["distill_t"], recorded["t2"], pred2="teacher_pred")
    _close(U.padded(inp, "v", torch.float32)["loss"], recorded, "loss_distill_v")
    _close(U.padded(inp, "v", torch.float32)["x_t"], recorded, "distill_x_t")
    _close(U.padded(inp, "distill", torch.float32)["loss"], recorded, "loss_distill")


def test_the_fixture_covers_the_ends_of_the_schedule(recorded):
    assert recorded["t1"].min() == 1 and recorded["t1"].max() == U.T_DIFF - 1
    assert int(recorded["distill_t"].max()) == U.T_DIFF - 1
    assert os.path.getsize(GOLDEN) < 512 * 1024


@pytest.mark.parametrize("kind", U.KINDS)
@pytest.mark.parametrize("name", ["O1", "O1-short", "O2-long"])
def test_ragged_oracle_on_full_lengths_is_the_padded_oracle(name, kind):
    inp = U.case(name)
    B, T, _ = inp["mel"].shape
    a = U.ragged(inp, kind, torch.float64, lengths=(T,) * B)
    b = U.padded(inp, kind, torch.float64)
    assert set(a) == set(b)
    for k in a:
        assert a[k].shape == b[k].shape, k
        assert float((a[k] - b[k]).abs().max()) <= 1e-12 * max(1.0, float(b[k].abs().max())), k


def test_the_cases_reach_what_they_are_for():
    chunk = 4096  # elements per (row, chunk) block of k_obj_loss (csrc/edtts_objective.h: kObjChunk)
    B, T, M = U.CASES["O1"][:3]
    assert (T * M) % 4 != 0 and min(U.CASES["O1"][3]) == 2
    B, T, M = U.CASES["O2"][:3]
    assert T * M > 2 * chunk and (T * M) % chunk != 0 and (T * M) % 4 == 0
    B, T, M = U.CASES["O3"][:3]
    assert (T * M) % 4 == 0 and (min(U.CASES["O3"][3]) * M) % 4 != 0
    assert U.CASES["O1-short"][4] == U.CASES["O1-short"][1] - 3 and U.CASES["O2-long"][4] == U.CASES["O2-long"][1] + 2
    for c in U.CASES.values():
        assert 1 in c[6] + c[7] and U.T_DIFF - 1 in c[6] + c[7]


# ---------------------------------------------------------------------------------------------- argument checks
@pytest.fixture()
def no_library(monkeypatch):
    """Any call into the library fails the test."""
    def boom():
        raise AssertionError("the library was called")
    monkeypatch.setattr(native, "lib", boom)


def test_bad_arguments_raise_before_any_library_call(no_library):
    sch = DiffusionSchedule(U.T_DIFF)
    with pytest.raises(ValueError, match="prediction"):
        DiffusionObjective(sch, prediction="x")
    obj = DiffusionObjective(sch)
    mel, t = torch.zeros(2, 5, 4), torch.tensor([1, 2])
    errors = (ValueError, native.EdttsError)
    with pytest.raises(errors, match="HIP device"):
        obj.prepare(mel, t, noise=torch.zeros(2, 5, 4))          # CPU tensors: there is no CPU path
    with pytest.raises(errors, match="dtype"):
        obj.prepare(mel.double(), t, seeds=[1, 2])
    with pytest.raises(errors, match="dtype"):
        obj.prepare(mel, t.int(), seeds=[1, 2])
    with pytest.raises(errors, match="expected 2 seeds"):
        obj.prepare(mel, t, seeds=[1, 2, 3])
    with pytest.raises(errors, match="shape"):
        obj.prepare(mel, t, noise=torch.zeros(2, 5, 3))
    with pytest.raises(errors, match="shape"):
        obj.prepare(mel, torch.tensor([1, 2, 3]), seeds=[1, 2])
    with pytest.raises(errors, match="statistics"):
        DiffusionObjective(sch, normalize=False).prepare(mel, t, seeds=[1, 2], stats=(torch.zeros(2, 1, 4), torch.ones(2, 1, 4)))
    with pytest.raises(errors, match="prediction='v'"):
        DiffusionObjective(sch, prediction="eps").distill_loss(mel, mel, None)


def test_losses_reject_cpu_and_wrong_dtype_predictions(no_library):
    obj = DiffusionObjective(DiffusionSchedule(U.T_DIFF))

    class Batch:
        B, T, M = 2, 5, 4
        mel = torch.zeros(2, 5, 4)

    class Prep:
        batch = Batch()

    errors = (ValueError, native.EdttsError)
    with pytest.raises(errors, match="HIP device"):
        obj.loss(torch.zeros(2, 5, 4), Prep())
    with pytest.raises(errors, match="dtype"):
        obj.loss(torch.zeros(2, 5, 4, dtype=torch.float16), Prep())
    with pytest.raises(errors, match="expected"):
        obj.loss(torch.zeros(2, 5, 3), Prep())


def test_the_module_is_exported_and_names_the_header_constants():
    import edge_diffusion_tts_amd as pkg
    assert pkg.DiffusionObjective is objective_module.DiffusionObjective and "DiffusionObjective" in pkg.__all__
    assert (native.EDTTS_OBJ_V, native.EDTTS_OBJ_EPS, native.EDTTS_OBJ_DISTILL, native.EDTTS_OBJ_CONSISTENCY) == (0, 1, 2, 3)
    assert native.OBJ_NOISE_STREAM == 0x54
