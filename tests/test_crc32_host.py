"""The CRC32 arithmetic of canvas_amd/csrc/crc32_block.hpp on the host, under AddressSanitizer and UndefinedBehaviorSanitizer: tests/crc32_host.cpp reads every case into
a heap buffer of exactly its size, cuts it into slices of every size the kernel may use, reduces the slices with the four tables and joins them with the shift operator.
A byte read past a case ends the program.  Everything is an integer: equality with zlib.crc32, for the sums and for the combine rule on concatenations."""
import os
import random
import shutil
import struct
import subprocess
import zlib

import pytest

from crc_cases import SLICE, blocks_of_every_length, fills

HERE = os.path.dirname(os.path.abspath(__file__))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("crc32_host")
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    # the runtimes linked statically where the compiler can: the program then runs whatever else the environment loads into a process
    for runtime in (["-static-libasan", "-static-libubsan"], []):
        p = subprocess.run([cxx] + SANITIZE + runtime + [str(probe), "-o", str(tmp / "probe")], capture_output=True, text=True)
        if p.returncode == 0:
            break
    else:
        pytest.skip("%s cannot link the sanitizer runtimes: %s" % (cxx, p.stderr.strip()[-200:]))
    exe = tmp / "crc32_host"
    p = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + SANITIZE + runtime + [os.path.join(HERE, "crc32_host.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return str(exe), tmp


def run(program, cases, pairs=()):
    """-> (slice sizes, shifted values, [(n, value per slice size ..., value as one slice)])"""
    exe, tmp = program
    path = tmp / "case.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<II", len(cases), len(pairs)) + b"".join(struct.pack("<II", c, n) for c, n in pairs) + b"".join(struct.pack("<I", len(c)) + c for c in cases))
    p = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-2000:])
    lines = p.stdout.splitlines()
    assert lines[0].startswith("slices ")
    sizes = [int(x) for x in lines[0].split()[1:]]
    shifts = [int(ln.split()[1]) for ln in lines if ln.startswith("shift ")]
    got = [tuple(int(x) for x in ln.split()[1:]) for ln in lines if ln.startswith("case ")]
    assert len(shifts) == len(pairs) and len(got) == len(cases)
    return sizes, shifts, got


def test_sliced_sums_equal_zlib(program):
    sizes = run(program, [])[0]
    assert sizes == [SLICE]          # the program says what the kernel uses; the lengths of crc_cases are built around it
    cases = blocks_of_every_length()
    sizes, _, got = run(program, [c[2] for c in cases])
    for (n, kind, data), values in zip(cases, got):
        want = zlib.crc32(data)
        assert values == (n,) + (want,) * (len(sizes) + 1), (n, kind, values, want)
    # on zeros the sum depends on the length alone: a wrong inversion or shift count cannot hide behind the data
    zeros = dict((n, v[1]) for (n, kind, _), v in zip(cases, got) if kind == "zeros")
    assert zeros[0] == 0 and zeros[1] == 0xD202EF8D and len(set(zeros.values())) == len(zeros)


def test_the_combine_rule_on_concatenations(program):
    rng = random.Random(7)
    trials = []
    for nb in (0, 1, 3, 4, 5, 1023, 1024, 65535, 65536):
        for na in (0, 1, 259, 4096):
            for kind in range(3):
                a, b = fills(na, rng)[kind][1], fills(nb, rng)[kind][1]
                trials.append((a, b))
    _, shifts, _ = run(program, [], [(zlib.crc32(a), len(b)) for a, b in trials])
    for (a, b), shifted in zip(trials, shifts):
        assert shifted ^ zlib.crc32(b) == zlib.crc32(a + b), (len(a), len(b))
    # the operator itself: nothing for no bytes, x^8 for one, and shifts add up
    _, s, _ = run(program, [], [(0x80000000, 0), (0x80000000, 1), (0x80000000, 65536), (0x12345678, 300), (0x12345678, 100), (0, 65536)])
    assert s[0] == 0x80000000 and s[1] == 0x00800000 and s[5] == 0
    _, t, _ = run(program, [], [(s[4], 200)])
    assert t[0] == s[3]
