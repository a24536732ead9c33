"""Host side of the ragged-batch plumbing (avse_challenge_amd/ragged.py): the lengths resolver, the pad helper and the
planned-run helper.  No GPU: the device of every tensor here is the CPU."""
import numpy as np
import pytest
import torch

from avse_challenge_amd import avse4, kernels, ragged

CPU = torch.device("cpu")


def test_a_a_lengths_object_comes_back_as_it_is_and_derives():
    lens = ragged.Lengths([4000, 2307, 16], CPU)
    assert ragged.as_lengths(lens, 3, 4000, CPU, "t") is lens and ragged.as_lengths(lens, 3, 4000, CPU, "t", True) is lens
    assert kernels.Lengths is ragged.Lengths and avse4.plan_ragged_batches is ragged.plan_ragged_batches
    frames = lens.map(lambda t: (t - 16) // 8 + 1)
    assert frames.host == (499, 287, 1) and frames.dev.dtype == torch.int32
    valid = ragged.Lengths([2, 0, 3], CPU).valid(3)
    assert valid.dtype == torch.bool and valid.tolist() == [[True, True, False], [False] * 3, [True] * 3]


@pytest.mark.parametrize("given", [[3, 7, 5], (3, 7, 5), np.array([3, 7, 5]), torch.tensor([3, 7, 5])])
def test_b_sequences_arrays_and_host_tensors_give_the_same_lengths(given):
    lens = ragged.as_lengths(given, 3, 7, CPU, "t")
    assert lens.host == (3, 7, 5) and all(type(v) is int for v in lens.host)
    assert lens.dev.dtype == torch.int32 and lens.dev.tolist() == [3, 7, 5]


@pytest.mark.parametrize("bad", [[3, 7], [3, 7, 5, 5], [3.5, 7, 5], [3, 8, 5], [0, 7, 5], [-1, 7, 5], [3, 2 ** 31, 5], []])
def test_c_bad_lengths_are_refused(bad):
    """A wrong count, a non-integer, a value outside [1, extent], one that does not fit int32, none at all."""
    for given in (bad, np.array(bad), torch.tensor(bad)):
        with pytest.raises(ValueError):
            ragged.as_lengths(given, 3, 7, CPU, "t")
    with pytest.raises(ValueError):
        ragged.as_lengths([3, 2 ** 31, 5], 3, 2 ** 40, CPU, "t")          # not the extent: the int32 device copy


def test_d_lo_0_admits_an_empty_row():
    lens = ragged.Lengths([0, 7, 5], CPU)
    assert lens.checked(3, 7, "t", lo=0) is lens and ragged.as_lengths([0, 7, 5], 3, 7, CPU, "t", True).host == lens.host
    for refused in (lambda: lens.checked(3, 7, "t"), lambda: ragged.as_lengths([0, 7, 5], 3, 7, CPU, "t"),
                    lambda: ragged.as_lengths([0, 8, 5], 3, 7, CPU, "t", True)):
        with pytest.raises(ValueError):
            refused()


def test_e_an_int32_tensor_on_the_device_passes_through():
    dev = torch.tensor([9, -1, 4], dtype=torch.int32)        # out of range: the kernel clamps, nothing is read back
    lens = ragged.as_lengths(dev, 3, 7, CPU, "t", clamped=True)
    assert lens.dev is dev and lens.host is None and ragged.as_lengths(lens, 3, 7, CPU, "t", clamped=True).dev is dev
    for bad in (dev.long(), dev.float(), dev[:2], dev[None]):
        with pytest.raises(ValueError):
            ragged.as_lengths(bad, 3, 7, CPU, "t", clamped=True)
    with pytest.raises(ValueError):                          # only the clamping entry points take what they cannot check
        ragged.as_lengths(lens, 3, 7, CPU, "t")


def test_g_pad_stack():
    a = [np.arange(1, n + 1, dtype=np.float32) for n in (5, 2, 3)]
    out, lens = ragged.pad_stack(a, 0)
    assert lens == [5, 2, 3] and out.dtype == np.float32 and out.shape == (3, 5)
    assert out.tolist() == [[1, 2, 3, 4, 5], [1, 2, 0, 0, 0], [1, 2, 3, 0, 0]]
    out, lens = ragged.pad_stack(a, -1, [2, 1])
    assert lens == [3, 2] and out.tolist() == [[1, 2, 3], [1, 2, 0]]
    g = np.random.default_rng(0)
    clips = [g.integers(1, 256, (3, t, 2, 2), dtype=np.uint8) for t in (5, 2, 3)]
    out, lens = ragged.pad_stack(clips, 1)
    assert lens == [5, 2, 3] and out.dtype == np.uint8 and out.shape == (3, 3, 5, 2, 2)
    for b, (c, t) in enumerate(zip(clips, lens)):
        assert np.array_equal(out[b, :, :t], c) and not out[b, :, t:].any()


def test_h_run_planned_returns_the_results_in_input_order():
    lengths, seen = [7, 3, 9, 3, 8], []

    def run(idx):
        seen.append(list(idx))
        return [(i, lengths[i]) for i in idx]
    assert ragged.run_planned(lengths, 2, 1.25, run) == [(i, n) for i, n in enumerate(lengths)]
    assert seen == ragged.plan_ragged_batches(lengths, 2, 1.25)
    assert sorted(i for idx in seen for i in idx) == [0, 1, 2, 3, 4] and max(len(idx) for idx in seen) <= 2
    with pytest.raises(ValueError):
        ragged.run_planned(lengths, 2, 1.25, lambda idx: [None])     # one result per index
    assert ragged.run_planned([], 2, 1.25, run) == []
