"""The frame table (zh_frame_table.cpp's build_frame_table) on blocks of several segments, without a GPU: tests/native/
solid_frame_table_main.cpp, a stand-alone program built with -fsanitize=address,undefined, plays the table of hand-made
blocks of several segments against a stream assembled byte by byte."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zpaqsharp_amd", "csrc")

WANT = ["ok one_segment", "ok one_segment_is_the_block_form", "ok empty_first_segment", "ok empty_last_segment", "ok empty_bodies",
        "ok 120_segments", "ok filenames_0_and_300", "ok no_sha1", "ok no_tag_later_batch", "ok pieces", "ok third_segment_does_not_fit"]


def test_solid_frame_table_in_a_sanitized_program(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed for the stand-alone check"
    exe = str(tmp_path / "solid_frame_table_main")
    # the sanitizers' runtime inside the program, so that it runs as it is wherever it is started; GCC and clang spell it differently
    about = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static = "-static-libsan" if "clang" in about else "-static-libasan"
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           static, "-I", CSRC, os.path.join(ROOT, "tests", "native", "solid_frame_table_main.cpp"),
                           os.path.join(CSRC, "zh_frame_table.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.split("\n")
    assert lines[:len(WANT)] == WANT and lines[len(WANT)].startswith("ok ") and lines[len(WANT)].endswith(" checks")
