"""Drop-in for the parts of mamba-ssm 1.1.3.post1 the reference imports."""


def __getattr__(name):
    # mamba_blocks.py:12 imports Mamba for its unidirectional (causal) configs: the project's mixer, resolved on
    # first use so that importing this package alone stays light
    if name == "Mamba":
        from avse_challenge_amd.mamba_tasnet import Mamba
        return Mamba
    raise AttributeError(name)
