"""Decode rate of the modelled LZ77 / BWT blocks with E8E9 (levels 3 and 4 on executables) with opts.kernel = KERNEL_MODEL_E8
(zh_nibble.hip runs their post-processor wave-wide, the end-of-segment E8E9 loop as rounds of zh_e8e9_wave.h) against the
default (kernel = 0: the program as translated code on one lane), and against each method's twin without E8E9, on the same
streams in one process.

    python3 tools/model_e8_rate.py [--blocks 256] [--kind X] [--rounds 2]

Streams: the CPU stream writer (synth.method_stream, 16 host threads), every block distinct; 256 KiB blocks for the two
level-3 methods, 64 KiB for level 4's single-ICM form (bench.py's method_streams sizes).  kernel = 0 and kernel = 11 are
ALTERNATED, --rounds times each, after one untimed warm-up decode per stream; one JSON line per run: kernel_ms
(zpaqhip_last_stats), plaintext MB/s from it, e8_wave_segs, and whether every byte equals the plaintext generator's (the
stored SHA-1 of every segment is verified too).  A summary line per method gives the best kernel_ms of kernel 0, kernel 11
and the twin, their ratios and the spread of the repeats."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import zpaqsharp_amd as z  # noqa: E402
from zpaqsharp_amd import method, synth  # noqa: E402

METHODS = (("level 3: lzpre + E8E9, icm/isse", "x0,6,12,0,7,16,1c0,0,511i2", "x0,2,12,0,7,16,1c0,0,511i2", 256),
           ("level 3: BWT + E8E9, icm/isse", "x0,7ci1", "x0,3ci1", 256),
           ("level 4: lzpre + E8E9, one icm", "x0,6,5,0,7,16,1c0,0,511", "x0,2,5,0,7,16,1c0,0,511", 64))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--blocks", type=int, default=256)
    p.add_argument("--kind", default="X")
    p.add_argument("--rounds", type=int, default=2)
    a = p.parse_args()
    print("# command: python3 tools/model_e8_rate.py " + " ".join(sys.argv[1:]), flush=True)
    K = z.KERNEL_MODEL_E8
    ctx = z.Context(0)
    for what, e8, twin, kib in METHODS:
        bs = kib << 10
        nbytes = a.blocks * bs
        want = np.concatenate([synth.plain(a.kind, b, bs) for b in range(a.blocks)])
        best = {}
        for form, name in (("e8e9", e8), ("twin", twin)):
            m, args = method.model_of(name)
            stream, _ = synth.method_stream(m, args, a.kind, a.blocks, bs, threads=16)
            ctx.decompress(stream, out_cap=nbytes)                                 # warm-up: arena allocation
            for rnd in range(a.rounds):
                for kernel in (0, K):
                    out = ctx.decompress(stream, out_cap=nbytes, kernel=kernel, verify_sha1=True)
                    st = ctx.stats()
                    ok = out.size == want.size and bool(np.array_equal(out, want))
                    print(json.dumps({"what": what, "form": form, "method": name, "kind": a.kind, "blocks": a.blocks, "block_size": bs,
                                      "coded_bytes": int(stream.size), "round": rnd, "kernel": kernel, "launches": st.launches,
                                      "e8_wave_segs": st.e8_wave_segs, "kernel_ms": st.kernel_ms, "MBps": nbytes / st.kernel_ms / 1e3,
                                      "all_equal": ok}), flush=True)
                    best.setdefault((form, kernel), []).append(st.kernel_ms)
        b = {k: min(v) for k, v in best.items()}
        print(json.dumps({"summary": what, "method": e8, "twin": twin, "MB": nbytes / 1e6,
                          "kernel0_ms": b[("e8e9", 0)], "kernel11_ms": b[("e8e9", K)], "twin_kernel0_ms": b[("twin", 0)], "twin_kernel11_ms": b[("twin", K)],
                          "kernel0_MBps": nbytes / b[("e8e9", 0)] / 1e3, "kernel11_MBps": nbytes / b[("e8e9", K)] / 1e3,
                          "twin_MBps": nbytes / b[("twin", 0)] / 1e3,
                          "kernel11_over_kernel0": b[("e8e9", 0)] / b[("e8e9", K)],      # how many times faster than the parent's path
                          "twin_over_kernel11": b[("e8e9", K)] / b[("twin", 0)],        # how many times slower than the twin without E8E9
                          "spread": {f"{f}_{k}": max(v) / min(v) - 1 for (f, k), v in best.items()}}), flush=True)


if __name__ == "__main__":
    main()
