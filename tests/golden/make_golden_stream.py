"""Golden outputs of the reference's STATEFUL (streaming) Mamba path -> tests/golden/mamba_stream.npz,
mamba_stack_stream.npz and manifest_stream.json.

Run on the build machine only (it imports the reference checkout named in make_golden.py; the GPU tests read
only the .npz files).  It reuses make_golden.py's import stubs and writes numbers only: the reference's
``Mamba.forward(hidden_states, inference_params)`` / ``step`` (bimamba.py:176-406) run in pure torch
(``selective_scan_fn = selective_scan_ref``, ``causal_conv1d_fn = causal_conv1d_update =
selective_state_update = None``), a prefill of PREFILL frames followed by single-frame steps.  Beside each
reference result the oracle's whole-sequence restatement (oracle/mamba_ref.py, no state at all) is compared and
the max-abs difference recorded, as make_golden.py does.

    python tests/golden/make_golden_stream.py
"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (puts the repository root on sys.path)
from oracle import mamba_ref  # noqa: E402
from oracle.det_init import det_init_, det_input  # noqa: E402

MANIFEST = {}
PREFILL, TOTAL = 9, 24


class _Params:
    """The caller-side state carrier (mamba_ssm.utils.generation.InferenceParams: the fields the reference reads)."""

    def __init__(self):
        self.seqlen_offset = 0
        self.key_value_memory_dict = {}


def _save(name, arrays, note, diffs):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **{k: v.detach().cpu().numpy() for k, v in arrays.items()})
    MANIFEST[name] = {"note": note, "oracle_vs_reference_maxabs": diffs, "bytes": os.path.getsize(path)}
    print(f"{name}: {diffs}")


def _stream(module, h, params):
    """prefill of PREFILL frames, then one frame at a time; returns the outputs and the states after the prefill"""
    with torch.no_grad():
        ys = [module(h[:, :PREFILL], inference_params=params)]
        params.seqlen_offset = PREFILL
        mid = {k: tuple(t.clone() for t in v) for k, v in params.key_value_memory_dict.items()}
        for t in range(PREFILL, h.shape[1]):
            ys.append(module(h[:, t:t + 1], inference_params=params))
            params.seqlen_offset += 1
    return torch.cat(ys, 1), mid


def _oracle_mixer(m, y):
    """forward-direction Mamba over the whole sequence from the oracle's pieces: (out, conv_state, ssm_state)"""
    r, n = m.dt_rank, m.d_state
    xz = F.linear(y, m.in_proj.weight).transpose(1, 2)
    xi, zi = xz.chunk(2, 1)
    b, _, l = xi.shape
    xc = mamba_ref.causal_conv1d(xi, m.conv1d.weight[:, 0], m.conv1d.bias, silu=True)
    xd = xc.transpose(1, 2).reshape(b * l, -1) @ m.x_proj.weight.t()
    dt = (m.dt_proj.weight @ xd[:, :r].t()).reshape(-1, b, l).transpose(0, 1)
    Bm = xd[:, r:r + n].reshape(b, l, n).transpose(1, 2)
    Cm = xd[:, r + n:].reshape(b, l, n).transpose(1, 2)
    out, last = mamba_ref.selective_scan(xc, dt, -torch.exp(m.A_log.float()), Bm, Cm, m.D.float(), zi,
                                         m.dt_proj.bias.float(), True, return_last_state=True)
    return F.linear(out.transpose(1, 2), m.out_proj.weight), xi[..., -m.d_conv:], last


def main():
    mg._install_stubs()
    ssi = mg._import_from("Mamba-TasNet", "modules.mamba.selective_scan_interface")
    bim = mg._import_from("Mamba-TasNet", "modules.mamba.bimamba")
    bim.selective_scan_fn = ssi.selective_scan_ref
    bim.causal_conv1d_fn = None
    bim.causal_conv1d_update = None
    bim.selective_state_update = None

    # ---- one mixer
    dm = 32
    ref_m = bim.Mamba(dm, bimamba_type="v2", use_fast_path=False, layer_idx=0)
    det_init_(ref_m, 11)
    h = det_input((2, TOTAL, dm), 201)
    params = _Params()
    y, mid = _stream(ref_m, h, params)
    conv_end, ssm_end = params.key_value_memory_dict[0]
    with torch.no_grad():
        y_stateless = ref_m(h)
        o_y, o_conv, o_ssm = _oracle_mixer(ref_m, h)
        _, o_conv_mid, o_ssm_mid = _oracle_mixer(ref_m, h[:, :PREFILL])
    _save("mamba_stream",
          dict(h=h, y=y, conv_state_prefill=mid[0][0], ssm_state_prefill=mid[0][1], conv_state_end=conv_end,
               ssm_state_end=ssm_end),
          f"bimamba.Mamba(32, bimamba_type='v2', use_fast_path=False, layer_idx=0), det_init seed 11, det_input "
          f"(2, {TOTAL}, 32) seed 201: forward(h[:, :{PREFILL}], inference_params) then {TOTAL - PREFILL} "
          "single-frame steps (bimamba.py:176-406, pure-torch fallbacks); states (2, 64, 4) and (2, 64, 16) after "
          "the prefill and after the last step",
          {"y": mg._maxabs(o_y, y), "y_vs_reference_stateless": mg._maxabs(y_stateless, y),
           "conv_state_prefill": mg._maxabs(o_conv_mid, mid[0][0]), "ssm_state_prefill": mg._maxabs(o_ssm_mid, mid[0][1]),
           "conv_state_end": mg._maxabs(o_conv, conv_end), "ssm_state_end": mg._maxabs(o_ssm, ssm_end)})

    # ---- two blocks
    mb = mg._import_from("Mamba-TasNet", "modules.mamba_blocks")
    mb.BiMamba = bim.Mamba
    ref_s = mb.MambaBlocksSequential(n_mamba=2, bidirectional=True, d_model=dm, rms_norm=True, fused_add_norm=False)
    det_init_(ref_s, 12)
    hs = det_input((2, TOTAL, dm), 202)
    params = _Params()
    ys, _ = _stream(ref_s, hs, params)
    with torch.no_grad():
        # oracle: the causal (forward-direction) stack over the whole sequence, Add -> RMSNorm -> mixer
        hcur, res, o_states = hs, None, []
        for layer in ref_s.layers:
            res = hcur + res if res is not None else hcur
            hcur, oc, os_ = _oracle_mixer(layer.mixer, mamba_ref.rms_norm(res, layer.norm.weight, layer.norm.eps))
            o_states.append((oc, os_))
        o_ys = mamba_ref.rms_norm(hcur + res, ref_s.norm_f.weight, ref_s.norm_f.eps)
    arrays, diffs = dict(h=hs, y=ys), {"y": mg._maxabs(o_ys, ys)}
    for i in range(2):
        c, s = params.key_value_memory_dict[i]
        arrays[f"conv_state_end_{i}"], arrays[f"ssm_state_end_{i}"] = c, s
        diffs[f"conv_state_end_{i}"] = mg._maxabs(o_states[i][0], c)
        diffs[f"ssm_state_end_{i}"] = mg._maxabs(o_states[i][1], s)
    _save("mamba_stack_stream", arrays,
          "mamba_blocks.MambaBlocksSequential(n_mamba=2, bidirectional=True, d_model=32, rms_norm=True, "
          f"fused_add_norm=False), det_init seed 12, det_input (2, {TOTAL}, 32) seed 202, with inference_params "
          f"(the BiMamba mixers then run their forward direction only): prefill of {PREFILL} frames then "
          f"{TOTAL - PREFILL} steps; output and both layers' final states",
          diffs)
    with open(os.path.join(HERE, "manifest_stream.json"), "w") as f:
        json.dump(MANIFEST, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
