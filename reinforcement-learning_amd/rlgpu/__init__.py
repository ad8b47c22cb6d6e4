"""rlgpu -- MI355X-native rollout engine for the GigaLearnCPP / RLGymCPP hot path.

Python mirror of the reference's operator surface over the C ABI in include/*.h.
"""
from ._lib import RLGPUError, LIB_PATH  # noqa: F401
from .gae import GAE  # noqa: F401


def __getattr__(name):
    if name == "InferUnit":  # rlgpu.InferUnit, imported on first use (it pulls in the env and PPO bindings)
        from .infer_unit import InferUnit
        return InferUnit
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
