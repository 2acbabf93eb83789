"""Forward E8E9 transform (LibZPAQ.cs:372-384): the pre-processor whose inverse is the E8E9 PCOMP of models.E8E9_PCOMP.

Product code for Context.compress_blocks with a `+e8e9` model (the CPU stream writer in synth / libzpaqgen is test
tooling).  The reference walks i = n-5 .. 0 and, where buf[i] is E8 or E9 and buf[i+4] is 00 or FF, adds i to the
24-bit little-endian operand buf[i+1..i+3].  A rewrite at i only touches bytes above i, so whether position i is a
candidate is decided by its original byte; only buf[i+4] can have changed when i is reached, and the loop below, which
visits the candidates from the top in the same order, sees it exactly as the reference does.
"""
from __future__ import annotations

import numpy as np


def forward(data) -> np.ndarray:
    a = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else data.view(np.uint8).reshape(-1)
    n = a.size
    out = bytearray(a.tobytes())
    if n < 5:
        return np.frombuffer(bytes(out), np.uint8).copy()
    cand = np.flatnonzero((a[:n - 4] & 254) == 0xE8)
    for i in cand[::-1].tolist():
        if ((out[i + 4] + 1) & 254) == 0:
            v = (out[i + 1] | out[i + 2] << 8 | out[i + 3] << 16) + i
            out[i + 1] = v & 255
            out[i + 2] = (v >> 8) & 255
            out[i + 3] = (v >> 16) & 255
    return np.frombuffer(bytes(out), np.uint8).copy()
