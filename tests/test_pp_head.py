"""zh_core.h's pp_head_step — PostProcessor.write's header states, the one copy the generic kernel runs — driven on the host in a
stand-alone C++ program built with -fsanitize=address,undefined (tests/native/pp_head_main.cpp), against a restatement of
PostProcessor.cs:37-79 written here.  No GPU, and no Python under a sanitizer."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zpaqsharp_amd", "csrc")
E_PP_EOS, E_PP_TYPE, E_PP_EMPTY = -8, -9, -10            # zh_model.h
MORE, LOADED = 0, 1


class Ref:
    """PostProcessor.write for states 0 and 2-4, case by case as the reference has them; errors are return values here."""

    def __init__(self, state=0, hsize=0, n=0):
        self.state, self.hsize, self.n, self.stores = state, hsize, n, 0

    def write(self, c):
        self.stores = 0
        if self.state == 0:
            if c < 0:
                return E_PP_EOS                          # "Unexpected EOS"
            self.state = c + 1
            if self.state > 2:
                return E_PP_TYPE                         # "unknown post processing type"
        elif self.state == 2:
            if c < 0:
                return E_PP_EOS
            self.hsize = c
            self.state = 3
        elif self.state == 3:
            if c < 0:
                return E_PP_EOS
            self.hsize += c * 256
            if self.hsize < 1:
                return E_PP_EMPTY                        # "Empty PCOMP"
            self.n = 0
            self.state = 4
        elif self.state == 4:
            if c < 0:
                return E_PP_EOS
            self.stores = 1                              # z.header[z.hend++] = c
            self.n += 1
            if self.n == self.hsize:
                self.state = 5
                return LOADED
        else:
            raise AssertionError("states 1 and 5 are not the header's")
        return MORE


def _expected():
    out = []

    def step(what, r, c):
        rc = r.write(c)
        out.append(f"{what} {c} -> {r.state} {r.hsize} {rc} {r.stores}")

    for c in range(256):
        step("first", Ref(), c)
    for c in range(256):
        step("low", Ref(2), c)
    for lo in (0, 255):
        for c in range(256):
            step("high255" if lo else "high0", Ref(3, lo), c)
    for what, r in (("eos0", Ref(0)), ("eos2", Ref(2)), ("eos3", Ref(3, 7)), ("eos4", Ref(4, 3, 1))):
        step(what, r, -1)
    for what, n in (("len1", 1), ("len65535", 65535)):
        r = Ref()
        step(what, r, 1)
        step(what, r, n & 255)
        step(what, r, n >> 8)
        for i in range(n):
            step(what, r, (i * 7 + 3) & 255)
        out.append(f"{what} stored {n} wrong 0 len {n}")
    r = Ref()
    for c in (1, 0, 0):
        step("len0", r, c)
    return out


def test_header_states_in_a_sanitized_program(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed for the stand-alone check of the header states"
    exe = str(tmp_path / "pp_head")
    about = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static = "-static-libsan" if "clang" in about else "-static-libasan"
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           static, "-I", CSRC, os.path.join(ROOT, "tests", "native", "pp_head_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got, want = r.stdout.split("\n")[:-1], _expected()
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w
    # what the sequence has to contain to mean anything: both selectors, the type error, the empty program, a load, every EOS
    text = r.stdout
    for line in ("first 0 -> 1 0 0 0", "first 1 -> 2 0 0 0", "first 2 -> 3 0 -9 0", "len0 0 -> 3 0 -10 0", "len1 3 -> 5 1 1 1",
                 "eos0 -1 -> 0 0 -8 0", "eos2 -1 -> 2 0 -8 0", "eos3 -1 -> 3 7 -8 0", "eos4 -1 -> 4 3 -8 0", "high255 255 -> 4 65535 0 0"):
        assert line in text, line
