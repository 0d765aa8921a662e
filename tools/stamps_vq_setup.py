#!/usr/bin/env python3
"""Set-up of the fused codebook search (csrc/vq_nearest.hip, stamps 6 / 7; -DISI_MEASURE build, see tools/stamps_convT.py)
inside the real forward at B = 64: the bottom search, workgroup 8, waves 0 and 4.  argv[1] = 1: the per-launch fill
(ISI_NO_SETUP_FUSION) instead of the pack-time image."""
import ctypes as C, os, pathlib, sys
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "interactive-spectrogram-inpainting_amd"))
os.environ.setdefault("ISI_HIP_LIBRARY", str(ROOT / "interactive-spectrogram-inpainting_amd" / "lib_measure" / "libisi_hip.so"))
import torch, bench
from interactive_spectrogram_inpainting import _hip
dev = torch.device("cuda:0")
model = bench._build_model(dev)[0]
x = torch.randn(64, 2, 128, 512, device=dev)
old = int(sys.argv[1]) if len(sys.argv) > 1 else 0
with torch.no_grad(), _hip.knob("ISI_NO_SETUP_FUSION", old):
    for _ in range(5): model(x)
    torch.cuda.synchronize()
    out = []
    for _ in range(5):
        model(x); torch.cuda.synchronize()
        buf = (C.c_longlong * 128)()
        assert _hip.lib().isi_debug_vq_stamps(buf, 128) == 0
        out.append((buf[7] - buf[6], buf[64 + 7] - buf[64 + 6], buf[5] - buf[0]))
print(f"knob {old}: bottom search in the forward, workgroup 8: (set-up wave 0, set-up wave 4, second tile) cycles: {out}")
