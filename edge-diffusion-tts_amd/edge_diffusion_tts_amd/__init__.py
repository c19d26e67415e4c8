"""edge_diffusion_tts_amd -- MI355X-native drop-in for the DDIM sampler path of Krabbens/edge-diffusion-tts.

Same public names as the reference package for this path (edge_diffusion_tts/__init__.py:17-21):
CFG, TrainPhase, get_device, set_seed, DiffusionSchedule, EdgeDiffusionDecoder, EdgeInference, SemanticEncoder, VectorQuantizer
(and FSQ, FSQEncoder of models/), plus the exported DepthwiseSeparableConv layer.  Everything numerical runs in libedtts_hip.so
(hand-written gfx950 kernels behind the C ABI of include/edtts.h); there is no CPU fallback.
"""
__version__ = "0.1.0"

from .config import CFG, TrainPhase, get_device, set_seed
from .schedule import DiffusionSchedule, DPMSolverPP
from .decoder import EdgeDiffusionDecoder
from .inference import EdgeInference
from .conv import DepthwiseSeparableConv
from .synth import synth_state_dict
from .longform import InpaintSampler
from .melpost import GriffinLim, InverseMelScale, MelVocoder, denormalize_mel, normalize_mel
from .encoder import FSQ, FSQEncoder, SemanticEncoder, VectorQuantizer
from .hubert import NativeHubert
from .audio import MelSpectrogram, Resample, chunk_stats_from_audio, resample
from .optim import FusedAdamW
from .objective import DiffusionObjective
from .graph_train import GraphedTrainStep, KeyStream

__all__ = [
    "CFG", "TrainPhase", "get_device", "set_seed", "DiffusionSchedule", "DPMSolverPP", "EdgeDiffusionDecoder", "EdgeInference",
    "DepthwiseSeparableConv", "synth_state_dict", "InpaintSampler",
    "GriffinLim", "InverseMelScale", "MelVocoder", "denormalize_mel", "normalize_mel",
    "SemanticEncoder", "VectorQuantizer", "FSQ", "FSQEncoder", "NativeHubert",
    "MelSpectrogram", "Resample", "resample", "chunk_stats_from_audio",
    "FusedAdamW", "DiffusionObjective", "GraphedTrainStep", "KeyStream",
]
