"""Dirty-memory helpers for the tests (a plain module: no test, no fixture).

A test process hands the kernels fresh driver memory, which reads as zero; a training run hands them recycled blocks
full of old activations.  ``dirty(monkeypatch)`` makes every ``torch.empty`` / ``empty_like`` / ``empty_strided`` of the
package's own modules come back filled with the 16-bit pattern 0x7FC0 over the whole storage (pads and slack
included): a NaN as fp16, as bf16 and -- doubled -- as fp32, and a large positive int32, so that a max word nobody
reset keeps it.  A kernel that reads what it never wrote then shows up as a NaN or as a difference from the clean run.
"""
import contextlib

import torch as _torch

POISON16 = 0x7FC0            # little-endian bytes C0 7F
POISON_TAIL = 0xC0           # an odd trailing byte
MODULES = ("kernels", "layers", "avse4", "mamba_tasnet")


def poison_(t):
    """Fill the whole storage under the freshly allocated tensor ``t`` (not only its logical elements) with POISON16;
    returns t."""
    st = t.untyped_storage()
    nb = st.nbytes()
    if nb == 0:
        return t
    raw = _torch.empty(0, dtype=_torch.uint8, device=t.device).set_(st, 0, (nb,), (1,))
    if nb >= 2:
        raw[:nb - (nb & 1)].view(_torch.int16).fill_(POISON16)
    if nb & 1:
        raw[nb - 1:].fill_(POISON_TAIL)
    return t


class PoisonTorch:
    """Stands in for the ``torch`` global of one module: everything is torch's, except that the three uninitialised
    allocators return poisoned memory."""

    def __init__(self, real_torch):
        self.__dict__["_real"] = real_torch

    def __getattr__(self, name):
        return getattr(self._real, name)

    def empty(self, *args, **kwargs):
        return poison_(self._real.empty(*args, **kwargs))

    def empty_like(self, *args, **kwargs):
        return poison_(self._real.empty_like(*args, **kwargs))

    def empty_strided(self, *args, **kwargs):
        return poison_(self._real.empty_strided(*args, **kwargs))


def package_modules():
    import importlib
    return [importlib.import_module("avse_challenge_amd." + m) for m in MODULES]


@contextlib.contextmanager
def dirty(monkeypatch):
    """Inside: kernels, layers, avse4 and mamba_tasnet allocate poisoned memory.  Undone on exit (and by monkeypatch's
    own teardown, should the body raise)."""
    with monkeypatch.context() as mp:
        for mod in package_modules():
            mp.setattr(mod, "torch", PoisonTorch(_torch))
        yield


@contextlib.contextmanager
def clean():
    """The counterpart of dirty(): the modules' own torch (so that one callable runs both ways in one loop)."""
    yield


def both(fn, monkeypatch):
    """(fn() under clean(), fn() under dirty(monkeypatch))."""
    with clean():
        a = fn()
    with dirty(monkeypatch):
        b = fn()
    return a, b
