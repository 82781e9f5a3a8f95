"""CPU-side checks of the CanvasSmooth surface: the three entry points are declared, listed and exported; the two host-only ones give the restatement's lengths
and a sensible plan; the executable is built by build_more_tools() and answers its command line the way CanvasSmooth's Program.Main does (Program.cs:23-67)
wherever no GPU is needed."""
import ctypes
import gzip
import os
import re
import subprocess

import numpy as np

import smooth_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("canvas_smooth", "canvas_smooth_lengths", "canvas_smooth_plan")
HELP = ["Usage: CanvasSmooth.exe [OPTIONS]+", "Smooth bin counts by repeated median filter", "", "Options:"]


def _exe():
    from canvas_amd import build
    build.build()
    exe = [e for e in build.build_more_tools() if os.path.basename(e) == "CanvasSmooth"]
    assert len(exe) == 1 and os.access(exe[0], os.X_OK)
    return exe[0]


def _run(args):
    return subprocess.run([_exe()] + args, capture_output=True, text=True, timeout=60)


def _body(stdout):
    """stdout without the echo of the command line (Utilities.LogCommandLine)"""
    lines = stdout.splitlines()
    assert lines[0] == ">>>Command-line arguments:"
    return lines[2:]


def test_symbols_declared_listed_and_exported():
    from canvas_amd import build
    from canvas_amd.lib import ABI_SYMBOLS
    so, _ = build.build()
    lib = ctypes.CDLL(so)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "canvas_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(canvas_\w+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in ABI_SYMBOLS and hasattr(lib, name), name
    assert "smooth.hip" in build.PRODUCT_SRC
    off = (ctypes.c_int64 * 2)(0, 4); out_n = (ctypes.c_int64 * 1)(0)
    assert lib.canvas_smooth(None, 1, off, None, 1, None, out_n) == -1        # no context: CANVAS_ERR_INVALID, nothing touched


def test_python_surface():
    from canvas_amd import Canvas, lib
    assert callable(Canvas.smooth) and callable(lib.smooth_lengths) and callable(lib.smooth_plan)


def test_lengths_equal_the_restatement():
    from canvas_amd.lib import smooth_lengths, CanvasError
    n = np.arange(0, 41)
    for W in range(0, 7):
        assert smooth_lengths(n, W).tolist() == [R.out_len(int(k), W) for k in n], W
    for W in (41, 100, 2**31 - 1):                       # larger than every chromosome
        assert smooth_lengths(n, W).tolist() == [0] * 41
    assert smooth_lengths([3_000_000, 2**31 - 1, 7], 3).tolist() == [3_000_000, 2**31 - 1, 7]
    assert smooth_lengths([], 3).tolist() == []
    for bad in (lambda: smooth_lengths([5], -1), lambda: smooth_lengths([-5], 1)):
        try:
            bad()
        except CanvasError:
            continue
        raise AssertionError("expected CANVAS_ERR_INVALID")


def test_plan():
    from canvas_amd.lib import smooth_plan, CanvasError
    for W in (1, 2, 3, 10):
        p = smooth_plan(W)
        assert p["fused"] and p["halo"] == W * (W + 1) // 2 and p["launches"] == 1
        assert p["tile"] >= 1024 and 2 * 4 * (p["tile"] + 2 * p["halo"]) <= 65536          # two float buffers of tile + halos within 64 KB
    huge = smooth_plan(100000)
    assert not huge["fused"] and huge["launches"] == 100000
    assert not smooth_plan(2**31 - 1)["fused"]
    assert smooth_plan(0)["launches"] == 0 and smooth_plan(0)["halo"] == 0
    try:
        smooth_plan(-1)
    except CanvasError:
        return
    raise AssertionError("expected CANVAS_ERR_INVALID")


def test_build_more_tools_builds_canvassmooth_and_build_tools_still_six():
    from canvas_amd import build
    exe = _exe()
    assert os.path.dirname(exe) == os.path.join(build.HERE, "bin")
    six = build.build_tools()
    assert len(six) == 6 and exe not in six
    assert build.embedded_hash(exe) is not None


def test_help_exits_0():
    for args in (["-h"], ["--help"], ["-i", "a", "-o", "b", "-h"]):
        r = _run(args)
        assert r.returncode == 0 and _body(r.stdout)[:4] == HELP, r.stdout
        assert "-w, --maxHalfWindowSize=VALUE" in r.stdout and "maximum half window size. Default: 0" in r.stdout


def test_missing_outfile_or_infile_prints_help_and_exits_1(tmp_path):
    for args in (["-i", str(tmp_path / "x.cleaned")], ["-o", str(tmp_path / "y")], []):
        r = _run(args)
        assert r.returncode == 1 and _body(r.stdout)[:4] == HELP, (args, r.stdout)


def test_missing_input_file_exits_1(tmp_path):
    src = str(tmp_path / "missing.cleaned"); out = tmp_path / "out.smoothed"
    r = _run(["-i", src, "-o", str(out), "-w", "2"])
    body = _body(r.stdout)
    assert r.returncode == 1 and body[0] == "CanvasSmooth.exe: File %s does not exist! Exiting." % src and body[1:5] == HELP
    assert not out.exists()


def test_unknown_argument_exits_0(tmp_path):
    r = _run(["-i", "a", "-o", "b", "--frobnicate"])
    body = _body(r.stdout)
    assert r.returncode == 0 and body[0] == "* Error: I don't understand the argument '--frobnicate'" and body[1:5] == HELP


def test_a_half_window_uint_parse_refuses_exits_nonzero(tmp_path):
    for w in ("-1", "abc", "1.5", "", "4294967296"):
        r = _run(["-i", "a", "-o", "b", "-w", w])
        assert r.returncode != 0 and "UInt32" in r.stderr, (w, r.stderr)
    r = _run(["-w", " +3 ", "-h"])                        # what uint.Parse accepts
    assert r.returncode == 0


def test_empty_input_needs_no_gpu(tmp_path):
    src = tmp_path / "empty.cleaned"; out = tmp_path / "empty.smoothed"
    with gzip.open(src, "wb"):
        pass
    r = _run(["-i", str(src), "-o", str(out), "-w", "3"])
    assert r.returncode == 0, r.stderr
    assert gzip.open(out, "rb").read() == b""
