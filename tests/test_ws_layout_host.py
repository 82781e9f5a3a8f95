"""The workspace layouts of canvas_amd/csrc/ws_layout.hpp on the host, under AddressSanitizer and UndefinedBehaviorSanitizer: tests/ws_layout_host.cpp measures
a layout, carves it into a heap block of exactly the measured size and writes every byte of every buffer.  A carve that runs past what was measured ends the
program — the check the GPU tests cannot make, because the device workspace is reserved with slack and a device allocation is rounded up."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("ws_layout_host")
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    # the runtimes linked statically where the compiler can: the program then runs whatever else the environment loads into a process
    for runtime in (["-static-libasan", "-static-libubsan"], []):
        p = subprocess.run([cxx] + SANITIZE + runtime + [str(probe), "-o", str(tmp / "probe")], capture_output=True, text=True)
        if p.returncode == 0:
            break
    else:
        pytest.skip("%s cannot link the sanitizer runtimes: %s" % (cxx, p.stderr.strip()[-200:]))
    exe = tmp / "ws_layout_host"
    p = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + SANITIZE + runtime + [os.path.join(HERE, "ws_layout_host.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return str(exe)


def expected_bytes():
    """takes of 0, 1, 255, 256, 257 elements of 1, 8 and 24 bytes, each starting on a 256-byte boundary: the end of the last one"""
    off = 0
    for size in (1, 8, 24):
        for n in (0, 1, 255, 256, 257):
            off = (off + 255) // 256 * 256 + n * size
    return off


def test_layouts(program):
    """empty layout, alignment / order / disjointness, measured == carved, every byte written, a refused reservation, a layout that differs between its
    passes, one layout on two bases — and not a word from either sanitizer, the measuring pass on a null base included"""
    p = subprocess.run([program], capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    n = expected_bytes()
    assert p.stdout.splitlines() == ["ok empty", "ok measure %d" % n, "ok carve %d" % n, "ok refused", "ok mismatch 0", "ok mismatch 1", "ok mirror"]


def test_a_write_past_the_measured_size_ends_the_program(program):
    p = subprocess.run([program, "overrun"], capture_output=True, text=True)
    assert p.returncode != 0 and "heap-buffer-overflow" in p.stderr, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    assert "went unnoticed" not in p.stdout
