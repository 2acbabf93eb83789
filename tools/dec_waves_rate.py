"""Decode rate of zh_chain.hip's run-time level walk with one decoder wave per compute unit (dec_waves=0, the kernel as it
was before the option) against the model's LDS plan of waves (api.dec_chain_plan), on the same streams in one process.

    python3 tools/dec_waves_rate.py [--blocks 1024] [--block-size 65536] [--kind T] [--rounds 2] [--kernel 4]
                                    [--models min,mid,x0,0ci1,1,1,1,2am | --level5]

Streams: the CPU stream writer (synth.stream / synth.method_stream, 16 host threads).  The two settings are ALTERNATED,
--rounds times each; one JSON line per run: kernel_ms (zpaqhip_last_stats), plaintext MB/s from it, the blocks in flight, and
whether the plaintext equals the first run's.  A last line per model gives the ratio of the best kernel_ms of each setting
and the spread between the rounds of one setting.  --models takes models names and method strings, separated by `;` when a
method string holds commas.  --level5: the model compressBlock writes for levels 5 to 9 (method.expand_level("5")), with
--kernel 0 (auto routes it to zh_chain)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import zpaqsharp_amd as z  # noqa: E402
from zpaqsharp_amd import api, method, models, synth  # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--blocks", type=int, default=1024)
    p.add_argument("--block-size", type=int, default=65536)
    p.add_argument("--kind", default="T")
    p.add_argument("--rounds", type=int, default=2)
    p.add_argument("--kernel", type=int, default=4)
    p.add_argument("--models", default="min;mid;x0,0ci1,1,1,1,2am")
    p.add_argument("--level5", action="store_true")
    a = p.parse_args()
    names = [method.expand_level("5", a.block_size, np.zeros(4096, np.uint32))] if a.level5 else a.models.split(";")
    kernel = 0 if a.level5 else a.kernel
    ctx = z.Context(0)
    nbytes = a.blocks * a.block_size
    for name in names:
        if name in models.NAMES:
            m = models.get(name)
            stream, _ = synth.stream(m, a.kind, a.blocks, a.block_size, threads=16)
        else:
            m, args = method.model_of(name)
            stream, _ = synth.method_stream(m, args, a.kind, a.blocks, a.block_size, threads=16)
        W = api.dec_chain_plan(m)[0]
        first, best = None, {}
        for rnd in range(a.rounds):
            for w in (0, W):
                out = ctx.decompress(stream, out_cap=nbytes, kernel=kernel, dec_waves=w)
                st = ctx.stats()
                if first is None:
                    first = out.copy()
                row = {"model": name, "kind": a.kind, "blocks": a.blocks, "block_size": a.block_size, "kernel": kernel, "round": rnd,
                       "dec_waves": w, "plan_waves": W, "in_flight": st.concurrent, "launches": st.launches, "kernel_kind": st.kernel_kind,
                       "kernel_ms": st.kernel_ms, "MBps": nbytes / st.kernel_ms / 1e3, "same_as_first": bool(np.array_equal(out, first))}
                print(json.dumps(row), flush=True)
                best.setdefault(w, []).append(st.kernel_ms)
        if W in best and 0 in best and W != 0:
            one, many = best[0], best[W]
            print(json.dumps({"model": name, "plan_waves": W, "one_wave_ms": min(one), "plan_ms": min(many),
                              "ratio": min(one) / min(many),
                              "spread_one_wave": max(one) / min(one) - 1, "spread_plan": max(many) / min(many) - 1}), flush=True)


if __name__ == "__main__":
    main()
