"""avse_challenge_amd — MI355X-native hot path of shangfuu/avse_challenge.

Hand-written gfx950 HIP kernels (libavse_hip.so, C ABI in include/avse_hip.h) behind the
reference's operator / module surfaces:
  kernels        torch wrappers of the C ABI (selective scan, causal conv1d, add+RMSNorm, STFT/iSTFT,
                 lip Conv3d weight gradient, PReLU, fused PReLU+gLN, depthwise dilated conv1d, BatchNorm+act,
                 max pooling, LSTM recurrence)
  layers         autograd modules over those kernels (PReLU, LipConv3d, prelu_gln, dwconv1d, dwconv_prelu_gln,
                 bn_act (BatchNorm -> [+res] -> act), maxpool3d, bn_act_pool_frames (the lip front-ends' fused
                 BatchNorm3d -> act -> MaxPool3d -> channels-last frames), HipLSTM)
  dropin         importable stand-ins for selective_scan_cuda / causal_conv1d(_cuda) / mamba_ssm
  mamba_tasnet   Mamba-TasNet separator (Encoder, MaskNet of BiMamba v2 blocks, Decoder)
  avse1          avse1 AVNet with the STFT front-end / iSTFT back-end on the GPU
  avse4          avse4 binaural AVSE4BaselineModule (TCN on the fused HIP kernels)
  losses, data   SI-SNR / PIT objectives; synthetic GPU-resident batches

miopen_db/ holds MIOpen find-db records (plain text, measured on MI355X with this image's MIOpen) for
the library convolutions the models keep on MIOpen.  Without them MIOpen's immediate mode evaluates
every candidate solver, naive ones included, on the first call of each shape: ~280 s for the avse1
B=32 step on a fresh box, vs ~8 s with the records.
"""
import os

MIOPEN_DB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "miopen_db")


def _miopen_user_db():
    """MIOpen appends the shapes it meets to its user find-db (and writes a .time file beside it): it gets a working
    copy of the committed records under build/ (beside the kernels' object files), so a run leaves the committed file
    as it is.  A record file is copied when the copy is missing or older; where build/ cannot be written, MIOpen
    reads the records in place."""
    import shutil
    dst = os.path.join(os.path.dirname(os.path.dirname(MIOPEN_DB)), "build", "miopen_db")
    try:
        os.makedirs(dst, exist_ok=True)
        for name in os.listdir(MIOPEN_DB):
            src, out = os.path.join(MIOPEN_DB, name), os.path.join(dst, name)
            if not os.path.exists(out) or os.path.getmtime(out) < os.path.getmtime(src):
                tmp = f"{out}.{os.getpid()}.tmp"
                shutil.copyfile(src, tmp)
                os.replace(tmp, out)                   # atomic: several ranks may start at once
    except OSError:
        return MIOPEN_DB
    return dst


if "MIOPEN_USER_DB_PATH" not in os.environ:
    os.environ["MIOPEN_USER_DB_PATH"] = _miopen_user_db()    # read by MIOpen at handle creation

# HIP graphs: the runtime's graph packet capture (ROCm 7.x CLR; AQL packets and kernel arguments prepared at
# instantiate time) replays some kernel nodes of the long single-stream avse1 train-step graph with the wrong
# arguments: reduction results land in each other's buffers (tools/avse1_graph_diag4.py @ 8f1eec2; loss -1.0 instead of
# 0.34).  With the capture off every replay matches the eager step.  Read at HIP runtime init, i.e. at the
# first GPU call, which comes after this import in every entry point (bench.py, tests, smoke()).
_PRESET = os.environ.get("DEBUG_CLR_GRAPH_PACKET_CAPTURE")
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")


def _graph_capture_safe():
    """False when the HIP runtime did (or will) start with graph packet capture on: the variable was set to
    something other than "0" by the caller, or a host program initialised the GPU before importing this package
    (then the setdefault above came too late).  ddp.Trainer.capture() then keeps the step eager."""
    import sys
    import warnings
    if _PRESET is not None and _PRESET != "0":
        warnings.warn("DEBUG_CLR_GRAPH_PACKET_CAPTURE is not 0: HIP-graph replay of the train steps is disabled")
        return False
    torch = sys.modules.get("torch")
    if _PRESET is None and torch is not None and torch.cuda.is_initialized():
        warnings.warn("the GPU was initialised before importing avse_challenge_amd, so DEBUG_CLR_GRAPH_PACKET_CAPTURE=0 "
                      "came too late: HIP-graph replay of the train steps is disabled (import the package first)")
        return False
    return True


GRAPH_CAPTURE_SAFE = _graph_capture_safe()

__version__ = "0.1.0"
