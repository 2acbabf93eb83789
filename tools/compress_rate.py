"""Compression rate of Context.compress_blocks against the CPU stream writer.

    python3 tools/compress_rate.py [--blocks 256] [--block-size 4194304] [--kinds T,R] [--model l1]

Per kind: plaintext MB/s from wall time, the time of each pass (zpaqhip_last_stats: init_ms = model pass, kernel_ms -
init_ms = coder pass), and the CPU writer
(synth.stream, 16 host threads) on the same blocks.  The outputs are compared byte for byte.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import zpaqsharp_amd as z  # noqa: E402
from zpaqsharp_amd import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=256)
    ap.add_argument("--block-size", type=int, default=1 << 22)
    ap.add_argument("--kinds", default="T,R")
    ap.add_argument("--model", default="l1")
    a = ap.parse_args()
    with z.Context(0) as ctx:
        for kind in a.kinds.split(","):
            blocks = [synth.plain(kind, i, a.block_size) for i in range(a.blocks)]
            mb = a.blocks * a.block_size / 1e6
            ctx.compress_blocks(a.model, blocks[:1])                     # warm-up
            t = time.perf_counter()
            got = ctx.compress_blocks(a.model, blocks)
            gpu_s = time.perf_counter() - t
            st = ctx.stats()
            t = time.perf_counter()
            want, _ = synth.stream(a.model, kind, nblocks=a.blocks, block_size=a.block_size, threads=16)
            cpu_s = time.perf_counter() - t
            print(json.dumps({"model": a.model, "kind": kind, "blocks": a.blocks, "block_size": a.block_size,
                              "gpu_MBps": mb / gpu_s, "gpu_wall_s": gpu_s, "kernel_ms": st.kernel_ms, "model_pass_ms": st.init_ms,
                              "coder_pass_ms": st.kernel_ms - st.init_ms, "launches": st.launches,
                              "kernel_kind": st.kernel_kind, "cpu16_MBps": mb / cpu_s, "ratio": len(got) / (mb * 1e6),
                              "identical": got == want.tobytes()}))


if __name__ == "__main__":
    main()
