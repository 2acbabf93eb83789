"""What solid blocks do to the ratio of small files, from the CPU oracle alone (the GPU writes the same bytes:
tests/test_gpu_solid.py): N files of S bytes of text, one file per block against the packing of compressor.pack_files into
solid blocks of the given sizes.

    python3 tools/solid_ratio.py [--files 4096] [--file-size 2048] [--models min,mid] [--block-sizes 65536,1048576]

One JSON line per model and form: the stream's bytes and its ratio to the plaintext.  Deterministic; no GPU needed."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import oracle  # noqa: E402
from tests import util  # noqa: E402
from zpaqsharp_amd import compressor, models  # noqa: E402


def solid_block(m, segs, names):
    c = oracle.Compressor(2 * sum(map(len, segs)) + 256 * len(segs) + len(m.header) + 65536)
    c.write_tag()
    c.start_block(m.header)
    for i, (s, n) in enumerate(zip(segs, names)):
        c.start_segment(n, str(len(s)).encode())
        if i == 0:
            c.post_process(m.pcomp or b"")
        c.compress(s)
        c.end_segment(oracle.sha1(s))
    c.end_block()
    return c.getvalue()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=4096)
    ap.add_argument("--file-size", type=int, default=2048)
    ap.add_argument("--models", default="min,mid")
    ap.add_argument("--block-sizes", default="65536,1048576")
    a = ap.parse_args()
    text = util.text(a.files * a.file_size, seed=41)
    files = [text[i * a.file_size:(i + 1) * a.file_size] for i in range(a.files)]
    names = [b"dir/file%05d.txt" % i for i in range(a.files)]
    for model in a.models.split(","):
        m = models.get(model)
        for bs in [0] + [int(x) for x in a.block_sizes.split(",")]:
            groups = [[i] for i in range(a.files)] if bs == 0 else compressor.pack_files([len(f) for f in files], bs)
            n = sum(len(solid_block(m, [files[i] for i in g], [names[i] for i in g])) for g in groups)
            print(json.dumps({"model": model, "files": a.files, "file_size": a.file_size, "form": "one file per block" if bs == 0 else "solid",
                              "block_size": bs or None, "blocks": len(groups), "stream_bytes": n, "ratio": n / len(text)}), flush=True)


if __name__ == "__main__":
    main()
