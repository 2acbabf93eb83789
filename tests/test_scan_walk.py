"""zh_scan_walk.h — the framing scan of a device-resident stream restated over two lists (tag hits, zero runs) — driven on the
host in a stand-alone C++ program built with -fsanitize=address,undefined (tests/native/scan_walk_main.cpp): the lists from a
plain loop, the walk as the GPU runs it (a parse per hit, the chain, the segment fill), every field and the error compared
with zh_framing.cpp's scan_stream on the cases of tests/scan_cases.py.  No GPU, and no Python under a sanitizer."""
import os
import shutil
import struct
import subprocess

import pytest

import zpaqsharp_amd as z
from tests import scan_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zpaqsharp_amd", "csrc")


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("scan_walk")
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed for the stand-alone check of the scan walk"
    exe = str(tmp / "scan_walk")
    about = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static = "-static-libsan" if "clang" in about else "-static-libasan"
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           static, "-I", CSRC, os.path.join(ROOT, "tests", "native", "scan_walk_main.cpp"),
                           os.path.join(CSRC, "zh_framing.cpp"), "-o", exe])
    path = tmp / "cases.bin"
    with open(path, "wb") as f:
        for name, s in sc.all_scan_cases():
            f.write(struct.pack("<I", len(name)) + name.encode() + struct.pack("<Q", len(s)) + s)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    out = r.stdout.split("\n")[:-1]
    assert r.returncode in (0, 1) and out, r.stdout[-2000:] + r.stderr[-4000:]
    return out


def test_the_walk_agrees_with_the_host_scan_on_every_case(lines):
    n = len(sc.all_scan_cases())
    assert lines[-1] == "%d cases, 0 failed" % n, "\n".join(x for x in lines if not x.startswith("ok "))
    assert [x.split()[1] for x in lines[:-1]] == [name for name, _ in sc.all_scan_cases()]


def test_the_cases_are_what_they_are_named_for(lines):
    """The streams exercise what they claim: the counts the program printed, and the host scan's verdict on the error cases."""
    info = {x.split()[1]: dict(kv.split("=") for kv in x.split()[2:7]) for x in lines[:-1]}
    assert int(info["framing/tiny_blocks"]["blocks"]) == 1600
    assert int(info["framing/mixed"]["blocks"]) == 6 and int(info["framing/segments"]["segs"]) == 6
    assert int(info["framing/bare_behind_255"]["blocks"]) == 4 and int(info["framing/bare_behind_255"]["tags"]) == 2
    assert int(info["framing/bare_start"]["blocks"]) == 2
    for k in range(1, 16):
        assert int(info["framing/gap_%d" % k]["blocks"]) == 3
    for name in ("payload_archive", "name_archive", "comment_archive", "coded_tag"):      # a tag hit inside a block
        assert int(info["framing/" + name]["tags"]) > int(info["framing/" + name]["blocks"]) == 2
    assert int(info["zeros/run_3"]["blocks"]) == 2 and int(info["zeros/run_3"]["rc"]) == 0
    assert int(info["zeros/run_to_end"]["rc"]) == -15 and int(info["zeros/no_run"]["rc"]) == -15
    assert int(info["zeros/chunk_past_end"]["rc"]) == -2
    for r in range(20):
        for fam in ("tag", "run4", "long"):
            assert int(info["boundary/%s_%d" % (fam, r)]["blocks"]) == 2
    for name, s, code, msg, kept, blk in sc.error_cases():
        got, err = z.scan(s, partial=True)
        assert got.n_blocks == kept and int(info["errors/" + name]["blocks"]) == kept
        if code == 0:
            assert err is None
            continue
        assert err is not None and err.block == blk
        if code is not None:
            assert err.code == code and msg in str(err)
