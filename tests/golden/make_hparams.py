"""Writes tests/golden/hparams/: the architecture settings of the reference's Mamba-TasNet / DPMamba hparams files.

Run:  python tests/golden/make_hparams.py <reference checkout>

For every saved `ckpts/WSJ0Mix/<family>_<size>/1234/hyperparams.yaml` (-> hparams/ckpts/<family>_<size>.yaml) and every
training recipe `hparams/WSJ0Mix/<family>_<size>.yaml` (-> hparams/recipes/<family>_<size>.yaml) of the reference's
Mamba-TasNet tree, the settings that describe the architecture are written back in the file's own format: the
top-level scalars avse_challenge_amd.ckpt_io.model_kwargs_from_hparams reads (with the `!ref` expressions they are
written as, and whatever those refer to) and the `Encoder` / `MaskNet` / `Decoder` entries with their hyperpyyaml tags.
Everything else (data paths, augmentation, optimiser, loggers) is left out.  tests/test_ckpt_io.py reads the result.
"""
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from avse_challenge_amd import ckpt_io  # noqa: E402

KEYS = ("N_encoder_out", "out_channels", "kernel_size", "kernel_stride", "num_spks", "ssm_dim", "mamba_expand",
        "mamba_conv", "n_dp", "chunk_size", "skip_around_intra", "n_mamba_dp", "n_mamba")
MODULES = ("Encoder", "MaskNet", "Decoder")
_REF = re.compile(r"<([A-Za-z_][A-Za-z0-9_]*)>")


def _scalar(v):
    if isinstance(v, bool):
        return "true" if v else "false"
    if isinstance(v, str) and "<" in v:
        return "!ref " + v
    return str(v)


def _emit(key, v, ind, out):
    pad = "  " * ind
    if isinstance(v, dict):
        d = dict(v)
        out.append(f"{pad}{key}: {d.pop('__tag__', '')}".rstrip())
        for k, x in d.items():
            _emit(k, x, ind + 1, out)
    else:
        out.append(f"{pad}{key}: {_scalar(v)}")


def reduce_file(src, dst, with_modules):
    hp = ckpt_io.read_hparams(src)
    keys, todo = [], [k for k in KEYS if k in hp]
    while todo:
        k = todo.pop(0)
        if k in keys:
            continue
        keys.append(k)
        if isinstance(hp[k], str):
            todo += [r for r in _REF.findall(hp[k]) if r in hp]
    out = []
    for k in sorted(keys, key=list(hp).index):
        _emit(k, hp[k], 0, out)
    if with_modules:
        for k in MODULES:
            _emit(k, hp[k], 0, out)
    os.makedirs(os.path.dirname(dst), exist_ok=True)
    with open(dst, "w") as f:
        f.write("\n".join(out) + "\n")
    assert ckpt_io.model_kwargs_from_hparams(dst) == ckpt_io.model_kwargs_from_hparams(src), src


def main():
    root = os.path.join(sys.argv[1], "Mamba-TasNet")
    for fam in ("mambatasnet", "dpmamba"):
        for size in ("XS", "S", "M", "L"):
            name = f"{fam}_{size}"
            reduce_file(os.path.join(root, "ckpts", "WSJ0Mix", name, "1234", "hyperparams.yaml"),
                        os.path.join(HERE, "hparams", "ckpts", name + ".yaml"), True)
            reduce_file(os.path.join(root, "hparams", "WSJ0Mix", name + ".yaml"),
                        os.path.join(HERE, "hparams", "recipes", name + ".yaml"), False)


if __name__ == "__main__":
    main()
