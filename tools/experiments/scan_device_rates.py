"""What the framing scan of a device-resident stream buys: for the two streams `bench.py --full` builds — 256 x 4 MiB of the
level-1 model, and the unmodelled `lzpre` method — the time of
  (a) zpaqhip_scan on a host copy,
  (b) a device-to-host copy of the stream plus (a): what a caller who holds the stream on the GPU has to do without
      zpaqhip_scan_device,
  (c) zpaqhip_scan_device,
  (d) decompress_device end to end, against zpaqhip_decompress host to host.
Every figure: three warm-up runs, then the median of seven, wall clock around a synchronised call (the calls return after
their stream work has completed); the scan's own kernel time (HIP events) is printed next to (c).

    python tools/experiments/scan_device_rates.py [--blocks 256] [--kib 4096] [--out profiles/scan_device/rates.txt]
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import zpaqsharp_amd as z  # noqa: E402
from tools import methods  # noqa: E402
from zpaqsharp_amd import models, synth  # noqa: E402

WARM, REPS = 3, 7


def timed(fn):
    for _ in range(WARM):
        fn()
    ts = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=256)
    ap.add_argument("--kib", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_device", "rates.txt"))
    ap.add_argument("--commit", default=None, help="the commit the tree is at, where the tool runs without the repository's history")
    args = ap.parse_args()
    nb, bs = args.blocks, args.kib << 10
    commit = args.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    lines = ["framing scan and decompression of device-resident streams; %d x %d KiB blocks of text-like plaintext" % (nb, args.kib),
             "parent commit %s + this change; %s; medians of %d runs after %d warm-up runs (min .. max)" % (
                 commit, torch.cuda.get_device_name(0), REPS, WARM)]
    with z.Context(0) as ctx:
        for label, build in (("level-1 model (single CM)", lambda: synth.stream(models.get("l1"), "T", nb, bs)[0]),
                             ("lzpre, no model (x2,2,12,0,7,22)", lambda: synth.method_stream(*methods.model_of("x2,2,12,0,7,22"), "T", nb, bs)[0])):
            s = np.ascontiguousarray(build())
            plain = nb * bs
            d_in = torch.from_numpy(s).cuda()
            pad = torch.zeros(64, dtype=torch.uint8, device="cuda")                      # (the stream's last dword stays readable)
            d_in = torch.cat([d_in, pad])
            host = np.empty(s.size, np.uint8)
            pinned = torch.from_numpy(host).pin_memory()
            d_out = torch.empty(plain + 64, dtype=torch.uint8, device="cuda")
            want = z.scan(s)
            got = ctx.scan_device(d_in.data_ptr(), s.size)
            same = [int(b.end_off) for b in want.blocks] == [int(b.end_off) for b in got.blocks] and want.n_segments == got.n_segments

            def dev_to_host_scan():
                pinned.copy_(d_in[:s.size])
                torch.cuda.synchronize()
                z.scan(pinned.numpy())

            a = timed(lambda: z.scan(s))
            b = timed(dev_to_host_scan)
            c = timed(lambda: ctx.scan_device(d_in.data_ptr(), s.size))
            c_kernel = float(ctx.stats().kernel_ms)
            c_launches = int(ctx.stats().launches)
            out_h = ctx.decompress(s, out_cap=plain)
            rc, n = ctx.decompress_device(d_in.data_ptr(), s.size, d_out.data_ptr(), plain)
            ok = rc == 0 and n == plain and np.array_equal(d_out[:n].cpu().numpy(), out_h)
            del out_h
            h = timed(lambda: ctx.decompress(s, out_cap=plain))
            d = timed(lambda: ctx.decompress_device(d_in.data_ptr(), s.size, d_out.data_ptr(), plain))
            st = ctx.stats()
            ms = lambda t: "%9.3f ms (%.3f .. %.3f)" % (t[0] * 1e3, t[1] * 1e3, t[2] * 1e3)
            lines += ["", "%s: stream %.1f MB, %d blocks, tables equal: %s, plaintext equal: %s" % (label, s.size / 1e6, want.n_blocks, same, ok),
                      "  (a) zpaqhip_scan, host copy                %s  %8.2f GB/s" % (ms(a), s.size / a[0] / 1e9),
                      "  (b) device -> pinned host copy + (a)       %s  %8.2f GB/s" % (ms(b), s.size / b[0] / 1e9),
                      "  (c) zpaqhip_scan_device                    %s  %8.2f GB/s   kernels %.3f ms in %d launches" % (
                          ms(c), s.size / c[0] / 1e9, c_kernel, c_launches),
                      "  (d) decompress_device, device to device    %s  %8.1f MB/s of plaintext   (kernel_ms %.1f, scan %.3f)" % (
                          ms(d), plain / d[0] / 1e6, st.kernel_ms, st.init_ms),
                      "      zpaqhip_decompress, host to host       %s  %8.1f MB/s of plaintext" % (ms(h), plain / h[0] / 1e6)]
            del d_in, d_out, pinned
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
