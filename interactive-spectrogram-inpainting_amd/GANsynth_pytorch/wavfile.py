"""RIFF/WAVE decoding with the standard library: what `SpectrogramsHelper.from_wavfile` and the upload route read
(the reference decodes with torchaudio / sox, absent here; reference flask_server.py:557-568, 624-667)."""
from __future__ import annotations

import struct

import torch


def read_wav(data: bytes):
    """RIFF/WAVE bytes -> (float32 mono tensor in [-1, 1], sampling rate): PCM 16-bit or IEEE float32, the two formats
    the reference's front end uploads (the reference decodes with torchaudio, absent here)."""
    if data[:4] != b"RIFF" or data[8:12] != b"WAVE":
        raise ValueError("not a RIFF/WAVE file")
    pos, fmt, payload = 12, None, None
    while pos + 8 <= len(data):
        tag, size = data[pos:pos + 4], struct.unpack("<I", data[pos + 4:pos + 8])[0]
        body = data[pos + 8:pos + 8 + size]
        if tag == b"fmt ":
            fmt = struct.unpack("<HHIIHH", body[:16])
        elif tag == b"data":
            payload = body
        pos += 8 + size + (size & 1)
    if fmt is None or payload is None:
        raise ValueError("WAVE file without fmt / data chunk")
    code, channels, rate, _, _, bits = fmt
    if code == 1 and bits == 16:
        x = torch.frombuffer(bytearray(payload[:len(payload) // 2 * 2]), dtype=torch.int16).float() / 32768.0
    elif code == 3 and bits == 32:
        x = torch.frombuffer(bytearray(payload[:len(payload) // 4 * 4]), dtype=torch.float32).clone()
    else:
        raise ValueError(f"unsupported WAVE encoding (format {code}, {bits} bits)")
    if channels > 1:
        x = x[:x.numel() // channels * channels].reshape(-1, channels).mean(1)
    return x, rate
