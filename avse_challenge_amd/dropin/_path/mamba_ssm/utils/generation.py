"""Drop-in for ``mamba_ssm.utils.generation.InferenceParams`` (the state carrier the reference's stateful
``Mamba.forward(hidden_states, inference_params)`` expects the caller to bring, bimamba.py:184-189,380-406)."""
from avse_challenge_amd.mamba_tasnet import InferenceParams  # noqa: F401
