"""Compression rate of Context.compress_blocks (or, with --method, Context.compress_method) against the CPU stream writer.

    python3 tools/compress_rate.py [--blocks 256] [--block-size 4194304] [--kinds T,R] [--model l1] [--method M] [--bwt] [--sa | --ht]
                                   [--level L [--analysis-only]] [--kernel 0] [--enc-waves 0] [--rounds 1] [--decode-kernel K] [--no-cpu]
                                   [--device] [--solid N]

Per kind: plaintext MB/s from wall time, the time of each pass (zpaqhip_last_stats: init_ms = model pass, kernel_ms -
init_ms = coder pass), and the CPU writer
(synth.stream, 16 host threads) on the same blocks.  The outputs are compared byte for byte.

--method M: Context.compress_method(M) against synth.method_stream (16 host threads, its own greedy hash parse, so the
ratios are compared, not the bytes); pre_ms = the device pre-processing (init_ms), encoder_ms = the rest of kernel_ms.
The GPU stream is checked by a round trip through Context.decompress(verify_sha1=True).  --bwt passes bwt=True, the
opt-in a level 3 method needs (its transform is unique, but the CPU writer is still compared by ratio only).  --sa runs
every call twice, without and with sa=True (the reference's suffix-array parse, for a level 1 / 2 method with
args[5] - args[0] >= 21), one line each with "sa" false / true; the CPU writer then makes the same parse (cpu16_*: its
suffix sort included), and its stream is compared with the sa=True one byte for byte ("identical").  --ht does the same
with ht=True (the reference's hash-table parse, for a level 1 / 2 method with args[5] - args[0] < 21), lines with "ht" false /
true.

--level L: a numeric method "LB,R,t" (Context.compress_level).  First the analysis of levels 5..9 on its own, whatever L is:
Context.gap_hist_blocks (kernel_ms, the host's copy times, wall time with the copies) against synth.gap_hist, the plain host
loop, on 1 and on 16 threads in this process, the histograms compared.  Then, unless --analysis-only, compress_level itself:
wall time, its split into analysis and encoding (Context.level_ms), the methods chosen, and a round trip through
Context.decompress(verify_sha1=True).  --kernel defaults to 2 here.

--model takes any models name (l1, min, mid, max, ...), --method any expanded method string, modelled ones included.
--kernel K[,K...]: the encoder choice (zpaqhip_compress_opts.kernel; 2 = lane-per-component encoder for chain models).
Several values are run ALTERNATED inside one process on the same blocks, --rounds times each, one JSON line per run, and
their outputs are compared with each other.  --enc-waves W[,W...] (with --model or --method): the lane-per-component encoder's
waves per compute unit (zpaqhip_compress_opts.enc_waves; 0 automatic, 1 one wave per unit as before the waves existed), several
values alternated in the same way, inside each --kernel value; "in_flight" is stats().concurrent.  --decode-kernel K adds the kernel time of Context.decompress of the stream
with that decoder kernel (4 = zh_chain.hip, level walk at run time).  --no-cpu skips the CPU writer and with it every
comparison with it (cpu16_MBps, identical, cpu16_ratio); the round trip and same_as_first remain.

--device (with --model, --method or --level): the host form (Context.compress_blocks / compress_method / compress_level) and
the device form (compress_blocks_device / compress_method_device / compress_level_device, whose rows also carry the gather
launch's own time and the scratch stream's bytes) on the same blocks, ALTERNATED in one process, --rounds times each
(default 2 here), one JSON line per call: wall time of the call, kernel_ms, launches.  The device form's input tensor is
filled before the clock starts and its output is compared with the host form's stream on the device ("identical").  A last
line gives the packing kernel's own rate for a method without a model (the store layout): there kernel_ms is the
pre-processing and the packing kernel and init_ms the pre-processing alone, so pack_ms = kernel_ms - init_ms of the device
form (best of the rounds), pack_GBps = stream bytes / pack_ms, and next to it d2d_GBps, a device-to-device copy of the same
number of bytes timed with events in the same process.  Behind a model the packing kernel's time is part of a kernel_ms
thousands of times as long and cannot be read off it: pack_ms is null.

--solid N (with --model): the cost of the encoders' segment loop.  Three forms on the same blocks, ALTERNATED in one process,
--rounds times each (default 2 here), one JSON line per call: Context.compress_blocks ("blocks"), Context.compress_solid with
every block as one segment ("solid1": the same bytes, "identical"), and with every block cut into N segments of equal
length ("solidN": N - 1 more end-of-segment bits and segment frames per block; checked by a round trip).
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


def decode_ms(ctx, a, stream):
    """kernel_ms of Context.decompress(stream) on the decoder kernel --decode-kernel names; nothing without one"""
    if a.decode_kernel is None:
        return {}
    ctx.decompress(stream, kernel=a.decode_kernel)
    st = ctx.stats()
    return {"decode_kernel": a.decode_kernel, "decode_kernel_ms": st.kernel_ms, "decode_kernel_kind": st.kernel_kind}


def run_method(ctx, a, kernels):
    model, args = method.model_of(a.method)
    for kind in a.kinds.split(","):
        blocks = [synth.plain(kind, i, a.block_size) for i in range(a.blocks)]
        mb = a.blocks * a.block_size / 1e6
        cpu = {}
        if not a.no_cpu:
            t = time.perf_counter()
            want, _ = synth.method_stream(model, args, kind, nblocks=a.blocks, block_size=a.block_size, threads=16, sa=a.sa, ht=a.ht)
            cpu = {"cpu16_MBps": mb / (time.perf_counter() - t), "cpu16_ratio": want.size / (mb * 1e6)}
        first = None
        for k in kernels:
            for sa in (False, True) if a.sa or a.ht else (False,):
                ctx.compress_method(a.method, blocks[:1], bwt=a.bwt, kernel=k, sa=sa and a.sa, ht=sa and a.ht)    # warm-up
        for rnd in range(a.rounds):
            for k, w, sa in [(k, w, sa) for k in kernels for w in a.waves for sa in ((False, True) if a.sa or a.ht else (False,))]:
                t = time.perf_counter()
                got = ctx.compress_method(a.method, blocks, bwt=a.bwt, kernel=k, sa=sa and a.sa, ht=sa and a.ht, enc_waves=w)
                gpu_s = time.perf_counter() - t
                st = ctx.stats()
                row = {"method": a.method, "kind": kind, "blocks": a.blocks, "block_size": a.block_size, "kernel": k, "round": rnd,
                       "enc_waves": w, "in_flight": st.concurrent, "ht" if a.ht else "sa": sa,
                       "gpu_MBps": mb / gpu_s, "gpu_wall_s": gpu_s, "kernel_ms": st.kernel_ms, "pre_ms": st.init_ms,
                       "encoder_ms": st.kernel_ms - st.init_ms, "launches": st.launches, "kernel_kind": st.kernel_kind,
                       "ratio": len(got) / (mb * 1e6)}
                if first is None or a.sa or a.ht:
                    first = got
                    back = ctx.decompress(got, verify_sha1=True)
                    row["round_trip"] = bool(back.size == a.blocks * a.block_size and all(
                        (back[i * a.block_size:(i + 1) * a.block_size] == blocks[i]).all() for i in range(a.blocks)))
                    row.update(decode_ms(ctx, a, got))
                else:
                    row["same_as_first"] = got == first
                if sa and cpu:
                    row["identical"] = got == want.tobytes()
                row.update(cpu)
                print(json.dumps(row), flush=True)


def run_device(ctx, a, kernels):
    import numpy as np
    import torch
    for kind in a.kinds.split(","):
        blocks = [synth.plain(kind, i, a.block_size) for i in range(a.blocks)]
        mb = a.blocks * a.block_size / 1e6
        in_off = np.arange(a.blocks + 1, dtype=np.uint64) * a.block_size
        d_in = torch.empty(a.blocks * a.block_size, dtype=torch.uint8, device="cuda")
        for i, b in enumerate(blocks):          # the generator is a host one: block by block, before any clock starts
            d_in[i * a.block_size:(i + 1) * a.block_size].copy_(torch.from_numpy(b))
        what = {"level": a.level} if a.level else {"method": a.method} if a.method else {"model": a.model}
        for k in kernels:
            def host(bl, k=k):
                if a.level:
                    return ctx.compress_level(a.level, bl, kernel=k, sa=a.sa, ht=a.ht)
                if a.method:
                    return ctx.compress_method(a.method, bl, bwt=a.bwt, kernel=k, sa=a.sa, ht=a.ht)
                return ctx.compress_blocks(a.model, bl, kernel=k)

            def device(n, d_out, k=k):
                if a.level:
                    return ctx.compress_level_device(a.level, d_in.data_ptr(), in_off[:n + 1], d_out.data_ptr(), d_out.numel(),
                                                     kernel=k, sa=a.sa, ht=a.ht)
                if a.method:
                    return ctx.compress_method_device(a.method, d_in.data_ptr(), in_off[:n + 1], d_out.data_ptr(), d_out.numel(),
                                                      bwt=a.bwt, kernel=k, sa=a.sa, ht=a.ht)
                return ctx.compress_blocks_device(a.model, d_in.data_ptr(), in_off[:n + 1], d_out.data_ptr(), d_out.numel(), kernel=k)

            want = host(blocks)                                              # warm-up of both forms, and the size
            d_want = torch.from_numpy(np.frombuffer(want, np.uint8).copy()).cuda()
            d_out = torch.empty(len(want) + 4096, dtype=torch.uint8, device="cuda")
            device(a.blocks, d_out)                                          # (the full shape: the first call of a size pays its allocations)
            store = bool(a.method) and not a.level and method.model_of(a.method)[0].header[6] == 0
            pack_ms = None
            for rnd in range(a.rounds):
                for form in ("host", "device"):
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    if form == "host":
                        got = host(blocks)
                        same = got == want
                    else:
                        rc, n, _ = device(a.blocks, d_out)
                    wall = time.perf_counter() - t
                    st = ctx.stats()
                    if form == "device":
                        same = bool(rc == 0 and n == len(want) and torch.equal(d_out[:n], d_want))
                    if form == "device" and store:
                        pack_ms = min(pack_ms or 1e30, st.kernel_ms - st.init_ms)
                    row = {**what, "kind": kind, "blocks": a.blocks, "block_size": a.block_size, "kernel": k, "form": form,
                           "round": rnd, "wall_s": wall, "MBps": mb / wall, "kernel_ms": st.kernel_ms, "pre_ms": st.init_ms,
                           "launches": st.launches, "out_bytes": st.out_bytes, "identical": same}
                    if a.level and form == "device":          # the mixed call's own figures: the gather launch, the scratch stream
                        row.update({"gather_ms": st.e8_wave_segs / 1e3, "scratch_bytes": st.model_bytes,
                                    "groups": len(set(ctx.level_methods))})
                    elif a.level:                             # the host form's statistics are its last group's: its wall time splits instead
                        row.update({"kernel_ms": None, "pre_ms": None, "launches": None, "out_bytes": len(got),
                                    "analysis_ms": ctx.level_ms["analysis"], "encode_ms": ctx.level_ms["encode"]})
                    print(json.dumps(row), flush=True)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            d2d = 1e30
            for _ in range(3):
                e0.record()
                d_out[:len(want)].copy_(d_want)
                e1.record()
                torch.cuda.synchronize()
                d2d = min(d2d, e0.elapsed_time(e1))
            print(json.dumps({**what, "kind": kind, "kernel": k, "stream_bytes": len(want), "pack_ms": pack_ms,
                              "pack_GBps": len(want) / 1e6 / pack_ms if pack_ms else None, "d2d_ms": d2d,
                              "d2d_GBps": len(want) / 1e6 / d2d}), flush=True)


def run_solid(ctx, a, kernels):
    n = a.solid
    for kind in a.kinds.split(","):
        blocks = [synth.plain(kind, i, a.block_size).tobytes() for i in range(a.blocks)]
        mb = a.blocks * a.block_size / 1e6
        step = (a.block_size + n - 1) // n
        cut = [[b[i:i + step] for i in range(0, len(b), step)] for b in blocks]
        forms = {"blocks": lambda k, w: ctx.compress_blocks(a.model, blocks, kernel=k, enc_waves=w),
                 "solid1": lambda k, w: ctx.compress_solid(a.model, [[b] for b in blocks], kernel=k, enc_waves=w),
                 f"solid{n}": lambda k, w: ctx.compress_solid(a.model, cut, kernel=k, enc_waves=w)}
        for k in kernels:
            ctx.compress_solid(a.model, cut[:1], kernel=k)                    # warm-up
        want, checked = {}, set()
        for rnd in range(a.rounds):
            for k, w, form in [(k, w, f) for k in kernels for w in a.waves for f in forms]:
                t = time.perf_counter()
                got = forms[form](k, w)
                wall = time.perf_counter() - t
                st = ctx.stats()
                row = {"model": a.model, "kind": kind, "blocks": a.blocks, "block_size": a.block_size, "kernel": k, "enc_waves": w,
                       "form": form, "segments_per_block": 1 if form != f"solid{n}" else len(cut[0]), "round": rnd, "wall_s": wall,
                       "MBps": mb / wall, "kernel_ms": st.kernel_ms, "kernel_MBps": mb / (st.kernel_ms / 1e3), "launches": st.launches,
                       "kernel_kind": st.kernel_kind, "in_flight": st.concurrent, "out_bytes": len(got), "ratio": len(got) / (mb * 1e6)}
                if form == "blocks":
                    want[k] = got
                elif form == "solid1":
                    row["identical"] = got == want[k]
                elif (k, form) not in checked:
                    checked.add((k, form))
                    row["round_trip"] = ctx.decompress(got, verify_sha1=True).tobytes() == b"".join(blocks)
                print(json.dumps(row), flush=True)


def run_level(ctx, a, kernels):
    for kind in a.kinds.split(","):
        blocks = [synth.plain(kind, i, a.block_size) for i in range(a.blocks)]
        mb = a.blocks * a.block_size / 1e6
        ctx.gap_hist_blocks(blocks[:1])                                     # warm-up
        row = {"level": a.level, "kind": kind, "blocks": a.blocks, "block_size": a.block_size}
        for rnd in range(a.rounds):
            t = time.perf_counter()
            hist = ctx.gap_hist_blocks(blocks)
            wall = time.perf_counter() - t
            st = ctx.stats()
            row.update({"round": rnd, "analysis_kernel_ms": st.kernel_ms, "analysis_h2d_ms": st.h2d_ms, "analysis_d2h_ms": st.d2h_ms,
                        "analysis_launches": st.launches, "analysis_wall_ms": wall * 1e3, "analysis_wall_MBps": mb / wall,
                        "analysis_kernel_MBps": mb / (st.kernel_ms / 1e3)})
            if not a.no_cpu:
                for th in (1, 16):
                    t = time.perf_counter()
                    want = synth.gap_hist(blocks, threads=th)
                    row[f"cpu{th}_ms"] = (time.perf_counter() - t) * 1e3
                row["identical"] = bool((hist == want).all())
            print(json.dumps(row), flush=True)
        if a.analysis_only:
            continue
        for k in kernels:
            ctx.compress_level(a.level, blocks[:1], kernel=k)                 # warm-up
        for rnd in range(a.rounds):
            for k in kernels:
                t = time.perf_counter()
                got = ctx.compress_level(a.level, blocks, kernel=k)
                gpu_s = time.perf_counter() - t
                methods = {}
                for m in ctx.level_methods:
                    methods[m] = methods.get(m, 0) + 1
                back = ctx.decompress(got, verify_sha1=True)
                print(json.dumps({"level": a.level, "kind": kind, "blocks": a.blocks, "block_size": a.block_size, "kernel": k,
                                  "round": rnd, "gpu_MBps": mb / gpu_s, "gpu_wall_s": gpu_s, "analysis_ms": ctx.level_ms["analysis"],
                                  "encode_ms": ctx.level_ms["encode"], "ratio": len(got) / (mb * 1e6), "methods": methods,
                                  "round_trip": bool(back.size == a.blocks * a.block_size and all(
                                      (back[i * a.block_size:(i + 1) * a.block_size] == blocks[i]).all() for i in range(a.blocks)))}),
                      flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=256)
    ap.add_argument("--block-size", type=int, default=1 << 22)
    ap.add_argument("--kinds", default="T,R")
    ap.add_argument("--model", default="l1")
    ap.add_argument("--method", default=None)
    ap.add_argument("--bwt", action="store_true", help="accept a level 3 (BWT) method")
    ap.add_argument("--sa", action="store_true", help="also run with sa=True (the reference's suffix-array parse)")
    ap.add_argument("--ht", action="store_true", help="also run with ht=True (the reference's hash-table parse)")
    ap.add_argument("--level", default=None, help='numeric method "LB,R,t" (Context.compress_level)')
    ap.add_argument("--analysis-only", action="store_true", help="with --level: only the gap histogram, GPU against the host loop")
    ap.add_argument("--kernel", default=None, help="encoder choice(s), comma separated; several are alternated (default 0; 2 with --level)")
    ap.add_argument("--enc-waves", default="0", help="chain encoder waves per compute unit, comma separated; several are alternated")
    ap.add_argument("--rounds", type=int, default=None, help="runs of each --kernel value (default 1; 2 with --device)")
    ap.add_argument("--device", action="store_true", help="host form against device form (compress_*_device), alternated")
    ap.add_argument("--solid", type=int, default=0, help="blocks, one-segment solid blocks and N-segment solid blocks, alternated")
    ap.add_argument("--decode-kernel", type=int, default=None, help="also time the decoder with this opts.kernel")
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU writer")
    a = ap.parse_args()
    kernels = [int(k) for k in (a.kernel or ("2" if a.level else "0")).split(",")]
    a.waves = [int(w) for w in a.enc_waves.split(",")]
    a.rounds = a.rounds if a.rounds is not None else 2 if a.device or a.solid else 1
    with z.Context(0) as ctx:
        if a.solid:
            return run_solid(ctx, a, kernels)
        if a.device:
            return run_device(ctx, a, kernels)
        if a.level:
            return run_level(ctx, a, kernels)
        if a.method:
            return run_method(ctx, a, kernels)
        for kind in a.kinds.split(","):
            blocks = [synth.plain(kind, i, a.block_size) for i in range(a.blocks)]
            mb = a.blocks * a.block_size / 1e6
            cpu, want = {}, None
            if not a.no_cpu:
                t = time.perf_counter()
                want = synth.stream(a.model, kind, nblocks=a.blocks, block_size=a.block_size, threads=16)[0].tobytes()
                cpu = {"cpu16_MBps": mb / (time.perf_counter() - t)}
            for k in kernels:
                ctx.compress_blocks(a.model, blocks[:1], kernel=k)       # warm-up
            first = None
            for rnd in range(a.rounds):
                for k, w in [(k, w) for k in kernels for w in a.waves]:
                    t = time.perf_counter()
                    got = ctx.compress_blocks(a.model, blocks, kernel=k, enc_waves=w)
                    gpu_s = time.perf_counter() - t
                    st = ctx.stats()
                    row = {"model": a.model, "kind": kind, "blocks": a.blocks, "block_size": a.block_size, "kernel": k, "round": rnd,
                           "enc_waves": w, "in_flight": st.concurrent, "gpu_MBps": mb / gpu_s, "gpu_wall_s": gpu_s, "kernel_ms": st.kernel_ms, "model_pass_ms": st.init_ms,
                           "coder_pass_ms": st.kernel_ms - st.init_ms, "launches": st.launches,
                           "kernel_kind": st.kernel_kind, "ratio": len(got) / (mb * 1e6)}
                    if want is not None:
                        row["identical"] = got == want
                    if first is None:
                        first = got
                        row.update(decode_ms(ctx, a, got))
                    else:
                        row["same_as_first"] = got == first
                    row.update(cpu)
                    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
