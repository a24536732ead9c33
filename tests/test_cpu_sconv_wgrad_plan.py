"""Host plan of the trunk 3x3 weight gradient (csrc/sconv.hip wg_setup): the partial-slab workspace that
avse_sconv_wgrad_workspace_bytes reports, for every trunk shape of both lip encoders.  No GPU.

The stride-1 shapes run the 9-tap kernel, whose workspace must not exceed the per-row plan's that it replaced; the
stride-2 shapes keep the per-row kernel and its plan.  The constants are the values of the per-row plan (ranges x
k-step groups x 9 co ci x 4 B), read from a build of the commit before the 9-tap kernel."""
import os

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "avse_challenge_amd", "libavse_hip.so")

needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libavse_hip.so not built (run __graft_entry__.build)")

# lip frames per step and trunk input sizes: avse1 (2400 frames, 24 x 24 trunk input), avse4 (2000 frames, 28 x 28)
MODELS = [(2400, (24, 12, 6, 3)), (2000, (28, 14, 7, 4))]
STRIDE1_CAP = {64: 100_859_904, 128: 101_449_728, 256: 103_809_024, 512: 113_246_208}      # ci = co
STRIDE2_PARENT = {64: 100_859_904, 128: 101_449_728, 256: 103_809_024}                      # ci -> 2 ci, both models


def _bytes(*a):
    from avse_challenge_amd import _lib
    return _lib.lib().avse_sconv_wgrad_workspace_bytes(*a)


@needs_lib
@pytest.mark.parametrize("frames,sizes", MODELS)
def test_stride1_workspace_within_the_per_row_plans(frames, sizes):
    for k, h in enumerate(sizes):
        c = 64 << k
        nb = _bytes(frames, h, h, c, c, 1)
        assert nb > 0, (frames, h, c)
        assert nb % (9 * c * c * 4) == 0, (frames, h, c, nb)          # whole partial slabs
        assert nb <= STRIDE1_CAP[c], (frames, h, c, nb)


@needs_lib
@pytest.mark.parametrize("frames,sizes", MODELS)
def test_stride2_workspace_unchanged(frames, sizes):
    for k, h in enumerate(sizes[:3]):
        c = 64 << k
        nb = _bytes(frames, h, h, c, 2 * c, 2)
        assert nb > 0, (frames, h, c)
        assert nb <= STRIDE2_PARENT[c], (frames, h, c, nb)


@needs_lib
def test_rows_too_wide_for_the_merged_stage_keep_a_plan():
    """Rows of 35 .. 90 pixels do not fit the 9-tap kernel's stage (two rows more than a kernel row's): the per-row
    kernel takes them, as before; 91 fit neither."""
    assert _bytes(2, 8, 48, 64, 64, 1) == 7_077_888
    assert _bytes(2, 8, 90, 64, 64, 1) == 13_565_952
    assert _bytes(2, 8, 91, 64, 64, 1) <= 0
