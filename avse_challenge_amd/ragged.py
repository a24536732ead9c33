"""Host-side plumbing of zero-padded ragged batches: the lengths of a batch, the plan that cuts a list
of utterances into padded batches, and the pad / run / scatter loop around one length-aware forward per batch.  torch
and numpy only; nothing here needs the GPU or the compiled library."""
import numpy as np
import torch


class Lengths:
    """Per-sample extents of a zero-padded ragged batch: the host values (validated without a device sync) and their
    int32 device copy, made once and handed to every length-aware launch of a forward.  host is None for lengths that
    exist on the device only (as_lengths with clamped=True): the kernels that take those clamp each value themselves."""

    def __init__(self, lengths, device):
        host = lengths.tolist() if hasattr(lengths, "tolist") else list(lengths)
        if not host or any(int(v) != v for v in host):
            raise ValueError(f"lengths must be a non-empty sequence of integers, got {host}")
        self.host = tuple(int(v) for v in host)
        if min(self.host) < -2 ** 31 or max(self.host) >= 2 ** 31:
            raise ValueError("lengths must fit int32")
        self.dev = torch.tensor(self.host, dtype=torch.int32, device=device)

    @classmethod
    def on_device(cls, dev):
        """The Lengths of an int32 device tensor, taken as it is: no value is read back."""
        self = cls.__new__(cls)
        self.host, self.dev = None, dev
        return self

    def map(self, fn):
        """The Lengths of fn(length) per sample (encoder frames, STFT frames, chunk counts): one more upload."""
        return Lengths([fn(v) for v in self.host], self.dev.device)

    def valid(self, n):
        """(B, n) bool: step t of sample b is one of its own (t < lengths[b])."""
        return torch.arange(n, device=self.dev.device)[None, :] < self.dev[:, None]

    def checked(self, batch, extent, what, lo=1):
        """self after the host check lo <= len <= extent for each of `batch` samples (ValueError otherwise)."""
        if self.host is None:
            raise ValueError(f"{what}: lengths are needed as host values (a sequence or a Lengths made from one)")
        if len(self.host) != batch:
            raise ValueError(f"{what}: {len(self.host)} lengths for a batch of {batch}")
        if min(self.host) < lo or max(self.host) > extent:
            raise ValueError(f"{what}: lengths must lie in [{lo}, {extent}], got [{min(self.host)}, {max(self.host)}]")
        return self


def as_lengths(lengths, batch, extent, device, what, clamped=False):
    """The Lengths of `batch` rows of `extent` steps on `device`, from whatever a caller holds: a Lengths (that same
    object, checked; nothing is uploaded again), or a sequence, an array or a host tensor (uploaded once).  Values lie
    in [1, extent].  clamped=True is for the entry points whose kernel clamps each value into the row
    (selective_scan_fwd, causal_conv1d_fwd, gln_cl_fwd): values in [0, extent], and an int32 tensor of `batch`
    entries already on the device passes through without a value being read back."""
    if isinstance(lengths, Lengths):
        if lengths.dev.device != device:
            raise ValueError(f"{what}: lengths live on {lengths.dev.device}, the tensors on {device}")
        if clamped and lengths.host is None:
            lengths = lengths.dev
        else:
            return lengths.checked(batch, extent, what, 0 if clamped else 1)
    if clamped and torch.is_tensor(lengths) and (lengths.is_cuda or lengths.device == device):
        if lengths.dtype != torch.int32 or tuple(lengths.shape) != (batch,) or lengths.device != device:
            raise ValueError(f"{what}: lengths must be {batch} int32 values on {device} (or a sequence), got "
                             f"{tuple(lengths.shape)} {lengths.dtype} on {lengths.device}")
        return Lengths.on_device(lengths.contiguous())
    return Lengths(lengths, device).checked(batch, extent, what, 0 if clamped else 1)


def plan_ragged_batches(lengths, batch_size, max_pad_ratio=1.25):
    """Batches for enhance_batch: the indices of `lengths` sorted by length and cut greedily so that a batch holds at
    most batch_size items and its padded size max(len) * n stays within max_pad_ratio of its useful size sum(len).
    Every index appears exactly once; an item no neighbour fits with is a batch of its own (ratio 1).  Host code; the
    ratio is a setting, not a claim about speed."""
    if batch_size < 1 or max_pad_ratio < 1.0:
        raise ValueError("plan_ragged_batches: batch_size >= 1 and max_pad_ratio >= 1")
    lengths = [int(v) for v in lengths]
    if any(v < 1 for v in lengths):
        raise ValueError("plan_ragged_batches: lengths must be positive")
    batches, cur, total = [], [], 0
    for i in sorted(range(len(lengths)), key=lambda j: (lengths[j], j)):
        n = lengths[i]                                       # ascending: the newcomer is the batch's longest
        if cur and (len(cur) == batch_size or n * (len(cur) + 1) > max_pad_ratio * (total + n)):
            batches.append(cur)
            cur, total = [], 0
        cur.append(i)
        total += n
    if cur:
        batches.append(cur)
    return batches


def pad_stack(arrays, axis, idx=None):
    """arrays[i] for i in idx (all of them by default), each zero-padded along `axis` to the longest and stacked on a
    new leading axis, in the arrays' dtype -> (the stacked array, the list of their lengths along axis)."""
    rows = [arrays[i] for i in (range(len(arrays)) if idx is None else idx)]
    lens = [r.shape[axis] for r in rows]
    shape = list(rows[0].shape)
    shape[axis] = max(lens)
    out = np.zeros((len(rows), *shape), rows[0].dtype)
    for r, (row, n) in enumerate(zip(rows, lens)):
        out[(r,) + (slice(None),) * (axis % row.ndim) + (slice(0, n),)] = row
    return out, lens


def run_planned(lengths, batch_size, max_pad_ratio, run):
    """run(idx) -> that batch's per-item results, for each batch idx of plan_ragged_batches(lengths, batch_size,
    max_pad_ratio); -> the results in input order."""
    out = [None] * len(lengths)
    for idx in plan_ragged_batches(lengths, batch_size, max_pad_ratio):
        for i, res in zip(idx, run(idx), strict=True):
            out[i] = res
    return out
