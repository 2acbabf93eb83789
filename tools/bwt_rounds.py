"""Device time of Context.bwt_blocks on one text block against the two blocks whose common prefixes are as long as the
block (one byte value, period 2): the suffix sort's rounds are bounded by log2(n), so the three stay within a small factor.

    python3 tools/bwt_rounds.py [--block-size 4194304]

Per block: kernel_ms and launches (zpaqhip_last_stats) of the second of two calls.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import zpaqsharp_amd as z  # noqa: E402
from zpaqsharp_amd import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--block-size", type=int, default=1 << 22)
    a = ap.parse_args()
    n = a.block_size
    with z.Context(0) as ctx:
        for name, d in (("text", synth.plain("T", 0, n).tobytes()), ("random", synth.plain("R", 0, n).tobytes()),
                        ("one_byte", b"z" * n), ("period_2", b"ab" * (n // 2))):
            ctx.bwt_blocks([d])
            ctx.bwt_blocks([d])
            st = ctx.stats()
            print(json.dumps({"block": name, "bytes": n, "kernel_ms": st.kernel_ms, "launches": st.launches}), flush=True)


if __name__ == "__main__":
    main()
