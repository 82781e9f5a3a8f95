"""The framing rules of canvas_amd/csrc/bam_frame.hpp on the host, under AddressSanitizer and UndefinedBehaviorSanitizer: tests/bam_frame_host.cpp reads a chunk
into a heap buffer of exactly its size, follows the block_size chain with the header's chain rule, classifies every record it reaches with the header's kinds, and
puts every offset of the chunk to the shape test.  A byte read past the chunk ends the program.  The classes, the offset the chain stops at and the sortedness state
are compared with tests/frame_ref.py, for the cases the GPU tests use (tests/frame_cases.py) under every rule."""
import os
import shutil
import struct
import subprocess

import pytest

import frame_cases as FC
import frame_ref as FR

HERE = os.path.dirname(os.path.abspath(__file__))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
T = 4096


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("bam_frame_host")
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    # the runtimes linked statically where the compiler can: the program then runs whatever else the environment loads into a process
    for runtime in (["-static-libasan", "-static-libubsan"], []):
        p = subprocess.run([cxx] + SANITIZE + runtime + [str(probe), "-o", str(tmp / "probe")], capture_output=True, text=True)
        if p.returncode == 0:
            break
    else:
        pytest.skip("%s cannot link the sanitizer runtimes: %s" % (cxx, p.stderr.strip()[-200:]))
    exe = tmp / "bam_frame_host"
    p = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + SANITIZE + runtime + [os.path.join(HERE, "bam_frame_host.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return str(exe), tmp


def run(program, buf, first, rule, state=(0, 0)):
    exe, tmp = program
    path = tmp / "case.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<QQiiiiqq", len(buf), first, *rule, *state) + bytes(buf))
    p = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-2000:])
    lines = p.stdout.splitlines()
    recs = [tuple(int(x) for x in ln.split()[1:]) for ln in lines if ln.startswith("rec ")]
    end = [int(x) for x in lines[-2].split()[1:]]
    shape = [int(x) for x in lines[-1].split()[1:]]
    assert lines[-2].startswith("end ") and lines[-1].startswith("shape")
    return recs, end, shape


def check(program, name, buf, first, rule, state=(0, 0, 0, 0)):
    recs, end, shape = run(program, buf, first, rule, state[:2])
    offs, info, after, seen = FR.frame(buf, first, rule, state)
    assert recs == seen, (name, rule)
    if len(buf) - first >= 4:
        assert end == [info[2], after[0], after[1] if after[0] else state[1], info[5]], (name, rule)
    return shape


def test_cases_under_every_rule(program):
    cases = FC.chunk_end_cases() + FC.tile_cases(T)[:-1] + FC.decoy_cases(T) + FC.hostile_cases(T)
    for name, buf, first in cases:
        for rule in FC.RULES.values():
            check(program, name, buf, first, rule)


def test_the_shape_test(program):
    """what the speculation looks for: every start of an ordinary record passes, zero bytes and the minimum record (no name) do not, and a decoy passes as well"""
    recs = FC.sorted_run(20, total=90)
    shape = check(program, "run", b"".join(recs), 0, FC.RULES["all"])
    assert shape == [90 * i for i in range(20)]
    assert check(program, "least", b"".join(FC.least(pos=i) for i in range(50)), 0, FC.RULES["all"]) == []
    name, buf, first = FC.decoy_cases(T)[1]
    shape = check(program, name, buf, first, FC.RULES["all"])
    offs = FR.frame(buf, first, FC.RULES["all"])[0]
    assert set(offs) <= set(shape) and T + 8 in shape and T + 8 not in offs
    # the last record of a chunk, whole to the byte, passes; one byte short it does not
    assert 90 * 19 not in check(program, "short", b"".join(recs)[:-1], 0, FC.RULES["all"])


@pytest.mark.parametrize("kind", [FR.ALL, FR.SNV, FR.HITS, FR.FRAGMENTS])
def test_random_streams_and_events(program, kind):
    rules = [r for r in FC.RULES.values() if r[0] == kind]
    for what, ev, code in [(None, None, FR.NONE)] + FC.events_of(kind):
        for where in ((0, 300) if ev is not None else (None,)):
            stream = FC.random_stream(11 + kind, kind, n=300, event=ev, where=where)
            buf = b"".join(stream)
            for rule in rules:
                check(program, what, buf, 0, rule)
                info = FR.frame(buf, 0, rule)[1]
                assert info[3] == code and (ev is None or info[0] == where + 1), (what, where, rule, info)


def test_sortedness_across_calls(program):
    a, b = b"".join(FC.sorted_run(10, start=100, total=80)), b"".join(FC.sorted_run(10, start=50, total=80))
    for rule in (FC.RULES["snv"], FC.RULES["hits_paired_sorted"]):
        flag = dict(flag=0x2) if rule[0] == FR.HITS else {}
        a, b = b"".join(FC.sorted_run(10, start=100, total=80, **flag)), b"".join(FC.sorted_run(10, start=50, total=80, **flag))
        offs, info, state, seen = FR.frame(a, 0, rule)
        assert info[3] == FR.NONE and state[:2] == [10, 127]
        check(program, "second call", b, 0, rule, state)
        offs, info, state2, seen = FR.frame(b, 0, rule, state)
        assert info[3] == FR.EV_UNSORTED and info[0] == 1 and info[5] == 127 and state2[:2] == [10, 127]
