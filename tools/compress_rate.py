"""Compression rate of Context.compress_blocks (or, with --method, Context.compress_method) against the CPU stream writer.

    python3 tools/compress_rate.py [--blocks 256] [--block-size 4194304] [--kinds T,R] [--model l1] [--method M] [--bwt]

Per kind: plaintext MB/s from wall time, the time of each pass (zpaqhip_last_stats: init_ms = model pass, kernel_ms -
init_ms = coder pass), and the CPU writer
(synth.stream, 16 host threads) on the same blocks.  The outputs are compared byte for byte.

--method M: Context.compress_method(M) against synth.method_stream (16 host threads, its own greedy hash parse, so the
ratios are compared, not the bytes); pre_ms = the device pre-processing (init_ms), encoder_ms = the rest of kernel_ms.
The GPU stream is checked by a round trip through Context.decompress(verify_sha1=True).  --bwt passes bwt=True, the
opt-in a level 3 method needs (its transform is unique, but the CPU writer is still compared by ratio only).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import zpaqsharp_amd as z  # noqa: E402
from zpaqsharp_amd import method, synth  # noqa: E402


def run_method(ctx, a):
    model, args = method.model_of(a.method)
    for kind in a.kinds.split(","):
        blocks = [synth.plain(kind, i, a.block_size) for i in range(a.blocks)]
        mb = a.blocks * a.block_size / 1e6
        ctx.compress_method(a.method, blocks[:1], bwt=a.bwt)              # warm-up
        t = time.perf_counter()
        got = ctx.compress_method(a.method, blocks, bwt=a.bwt)
        gpu_s = time.perf_counter() - t
        st = ctx.stats()
        t = time.perf_counter()
        want, _ = synth.method_stream(model, args, kind, nblocks=a.blocks, block_size=a.block_size, threads=16)
        cpu_s = time.perf_counter() - t
        back = ctx.decompress(got, verify_sha1=True)
        ok = back.size == a.blocks * a.block_size and all(
            (back[i * a.block_size:(i + 1) * a.block_size] == blocks[i]).all() for i in range(a.blocks))
        print(json.dumps({"method": a.method, "kind": kind, "blocks": a.blocks, "block_size": a.block_size,
                          "gpu_MBps": mb / gpu_s, "gpu_wall_s": gpu_s, "kernel_ms": st.kernel_ms, "pre_ms": st.init_ms,
                          "encoder_ms": st.kernel_ms - st.init_ms, "launches": st.launches, "kernel_kind": st.kernel_kind,
                          "cpu16_MBps": mb / cpu_s, "ratio": len(got) / (mb * 1e6), "cpu16_ratio": want.size / (mb * 1e6),
                          "round_trip": bool(ok)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=256)
    ap.add_argument("--block-size", type=int, default=1 << 22)
    ap.add_argument("--kinds", default="T,R")
    ap.add_argument("--model", default="l1")
    ap.add_argument("--method", default=None)
    ap.add_argument("--bwt", action="store_true", help="accept a level 3 (BWT) method")
    a = ap.parse_args()
    with z.Context(0) as ctx:
        if a.method:
            return run_method(ctx, a)
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
