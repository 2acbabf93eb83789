"""Decode rate of unmodelled LZ77 blocks with E8E9 on zh_store.hip (opts.kernel = KERNEL_STORE_E8: the end-of-segment pass
runs wave-wide, zh_e8e9_wave.h) against the default (kernel = 0: the store kernel hands such a block to zh_generic.hip in a
second launch), and against the method's twin without E8E9, on the same streams in one process.

    python3 tools/store_e8_rate.py [--blocks 256] [--block-size 4194304] [--kind X] [--rounds 2] [--level 1] [--walk-blocks 16]

Method: what method.expand_level gives for the level at type "exe" (redundancy 128) and a block of that size, and the same
at type "binary".  Streams: the CPU stream writer (synth.method_stream, 16 host threads), every block distinct.  kernel = 0
and kernel = 10 are ALTERNATED, --rounds times each; one JSON line per run: kernel_ms (zpaqhip_last_stats), plaintext MB/s
from it, launches, and the bytes that equal the plaintext generator's (bytes_checked; SHA-1 of every segment is verified
too).  Summary lines give the ratios of the best kernel_ms.  Last, the schedule of zh_e8e9_wave.h is played on the host (the
harness of tests/e8w_harness.py, needs g++) over what the LZ77 codes of the first --walk-blocks blocks write, and its
rounds, walk passes per round and positions walked per byte are printed."""
import argparse
import ctypes
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import zpaqsharp_amd as z  # noqa: E402
from zpaqsharp_amd import method, synth  # noqa: E402


def walk_stats(kind, blocks, block_size):
    from tests import e8w_harness
    with tempfile.TemporaryDirectory() as d:
        lib, _ = e8w_harness.compile_lib(d, "-O2")
        tot = np.zeros(4, np.uint64)
        for b in range(blocks):
            m = synth.e8e9(synth.plain(kind, b, block_size)).copy()        # what the segment's codes write into M
            out = np.empty(max(1, m.size), np.uint8)
            stat = (ctypes.c_uint64 * 4)()
            rc = lib.e8w_pass(m.ctypes.data, m.ctypes.data, out.ctypes.data, m.size, m.size, stat)     # (zh_store.hip's call: M in place)
            assert rc == 0
            assert np.array_equal(out, synth.plain(kind, b, block_size))
            tot[0] += stat[0]; tot[1] += stat[1]; tot[3] += stat[3]
            tot[2] = max(int(tot[2]), int(stat[2]))
        return {"walk_blocks": blocks, "rounds": int(tot[0]), "passes_per_round": float(tot[1]) / max(1, int(tot[0])),
                "most_passes_in_a_round": int(tot[2]), "positions_walked_per_byte": float(tot[3]) / max(1, blocks * block_size)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--blocks", type=int, default=256)
    p.add_argument("--block-size", type=int, default=4 << 20)
    p.add_argument("--kind", default="X")
    p.add_argument("--rounds", type=int, default=2)
    p.add_argument("--level", default="1")
    p.add_argument("--walk-blocks", type=int, default=16)
    a = p.parse_args()
    print("# command: python3 tools/store_e8_rate.py " + " ".join(sys.argv[1:]), flush=True)
    names = {"e8e9": method.expand_level(f"{a.level},128,2", a.block_size), "plain": method.expand_level(f"{a.level},128,0", a.block_size)}
    ctx = z.Context(0)
    nbytes = a.blocks * a.block_size
    want = np.concatenate([synth.plain(a.kind, b, a.block_size) for b in range(a.blocks)])
    best = {}
    for form, name in names.items():
        m, args = method.model_of(name)
        stream, _ = synth.method_stream(m, args, a.kind, a.blocks, a.block_size, threads=16)
        for rnd in range(a.rounds):
            for kernel in (0, z.KERNEL_STORE_E8):
                out = ctx.decompress(stream, out_cap=nbytes, kernel=kernel, verify_sha1=True)
                st = ctx.stats()
                ok = int(np.count_nonzero(out == want)) if out.size == want.size else 0
                print(json.dumps({"form": form, "method": name, "kind": a.kind, "blocks": a.blocks, "block_size": a.block_size,
                                  "coded_bytes": int(stream.size), "round": rnd, "kernel": kernel, "launches": st.launches,
                                  "kernel_ms": st.kernel_ms, "MBps": nbytes / st.kernel_ms / 1e3, "bytes_checked": ok,
                                  "all_equal": ok == nbytes}), flush=True)
                best.setdefault((form, kernel), []).append(st.kernel_ms)
    b = {k: min(v) for k, v in best.items()}
    K = z.KERNEL_STORE_E8
    print(json.dumps({"e8e9_kernel0_ms": b[("e8e9", 0)], "e8e9_kernel10_ms": b[("e8e9", K)], "plain_kernel0_ms": b[("plain", 0)],
                      "plain_kernel10_ms": b[("plain", K)],
                      "kernel10_over_kernel0": b[("e8e9", 0)] / b[("e8e9", K)],          # how many times faster than the parent's path
                      "plain_twin_over_kernel10": b[("e8e9", K)] / b[("plain", K)],     # how many times slower than the twin without E8E9
                      "spread": {f"{f}_{k}": max(v) / min(v) - 1 for (f, k), v in best.items()}}), flush=True)
    if a.walk_blocks:
        print(json.dumps(walk_stats(a.kind, min(a.walk_blocks, a.blocks), a.block_size)), flush=True)


if __name__ == "__main__":
    main()
