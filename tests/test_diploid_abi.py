"""CPU-side checks of the CanvasDiploidCaller surface that is built so far: canvas_segment_select and its plan are declared, listed and exported, the plan is sensible, and
the select refuses bad arguments before it touches the device (no GPU here: a call that got as far as the device would fail with a HIP error instead)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("canvas_segment_select", "canvas_segment_select_plan", "canvas_call_diploid")
INVALID = -1


@pytest.fixture(scope="module")
def lib():
    from canvas_amd import build
    so, _ = build.build()
    lib = ctypes.CDLL(so)
    lib.canvas_segment_select.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def test_symbols_declared_listed_and_exported(lib):
    from canvas_amd import build
    from canvas_amd.lib import ABI_SYMBOLS
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "canvas_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(canvas_\w+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in ABI_SYMBOLS and hasattr(lib, name), name
    assert "call.hip" in build.PRODUCT_SRC
    cs = open(os.path.join(ROOT, "hosts", "CanvasHip.cs")).read()
    for name in NEW:
        assert re.search(r"extern int %s\(" % name, cs), name


def test_python_surface():
    from canvas_amd import Canvas, lib
    assert callable(Canvas.segment_select) and callable(lib.segment_select_plan) and callable(Canvas.call_diploid)
    assert lib.LOGISTIC_GERMLINE == (-5.0123, 4.9801, -5.5472, -1.7914) and (lib.FILTER_Q10, lib.FILTER_L10KB) == (1, 2)
    assert (lib.SELECT_MEDIAN_F32, lib.SELECT_MEDIAN_F64, lib.SELECT_UPPER) == (0, 1, 2)


def test_plan():
    from canvas_amd.lib import segment_select_plan
    p = segment_select_plan()
    assert p["wave_max"] == 64                                                   # one wave
    assert p["wave_max"] < p["lds_max"] and 4 * p["lds_max"] + 2 * 1024 <= 160 * 1024 // 4       # keys + two histogram rows, four workgroups in the 160 KiB of a CU
    assert p["tile"] >= 1024 and p["launches"] <= 16 and p["forced"] is None


def test_the_hook_is_seen_by_the_plan(monkeypatch):
    from canvas_amd.lib import segment_select_plan
    assert os.environ.get("CANVAS_TEST_HOOKS")                                   # tests/conftest.py
    for name in ("wave", "lds", "tiled"):
        monkeypatch.setenv("CANVAS_CALL_CLASS", name)
        assert segment_select_plan()["forced"] == name
    monkeypatch.setenv("CANVAS_CALL_CLASS", "frobnicate")
    assert segment_select_plan()["forced"] is None


def test_select_refuses_bad_offsets_before_it_looks_at_the_context(lib):
    """the offsets and the mode are checked first: with no context at all, *h_nempty is written exactly when they have passed"""
    def call(off, mode):
        o = np.array(off, np.int64); nempty = ctypes.c_int64(-7)
        rc = lib.canvas_segment_select(None, None, len(o) - 1, o.ctypes.data, mode, None, ctypes.byref(nempty))
        return rc, nempty.value
    assert call([0, 4, 4, 9], 0) == (INVALID, 1) and call([3, 3], 2) == (INVALID, 1)          # good tables: refused for the missing context only
    for off, mode in (([0, 5, 4, 8], 0), ([-1, 4], 0), ([0, 4], 3), ([0, 4], -1)):
        assert call(off, mode) == (INVALID, -7), (off, mode)
    assert lib.canvas_segment_select(None, None, 1, None, 0, None, None) == INVALID
    assert lib.canvas_segment_select_plan(None) == INVALID


def _call_diploid_tables(**change):
    t = dict(nbins=10, nchr=2, cso=[0, 2, 3], beg=[0, 100, 0], end=[100, 200, 50], sbo=[0, 4, 7, 10], csi=[0, 0, 0])
    t.update(change)
    return t


def _call_diploid_without_context(lib, t):
    A = lambda v, d: np.array(v, d)
    cso, beg, end, sbo, csi = A(t["cso"], np.int64), A(t["beg"], np.int32), A(t["end"], np.int32), A(t["sbo"], np.int64), A(t["csi"], np.int64)
    b4 = np.zeros(4, np.float64); n = max(len(beg), 1)
    f8 = lambda: np.zeros(n + 1, np.float64); i8 = lambda: np.zeros(n + 1, np.int64); i4 = lambda: np.zeros(n + 1, np.int32)
    outs = [f8(), i8(), i4(), f8(), i4(), i4(), f8(), f8(), i4()]
    runs = [i8(), i8(), i4(), i4(), f8()]
    nruns = ctypes.c_int64(-7); scal = np.zeros(2, np.float64)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    one = ctypes.c_void_p(64)                                  # stands for a device pointer: never dereferenced on the host
    lib.canvas_call_diploid.argtypes = None
    rc = lib.canvas_call_diploid(None, ctypes.c_int64(t["nbins"]), one, ctypes.c_int32(t["nchr"]), P(cso), P(beg), P(end), P(sbo), P(csi), one, one, one, P(b4),
                                 *[P(a) for a in outs], ctypes.byref(nruns), *[P(a) for a in runs], P(scal), None)
    return rc, nruns.value


def test_call_diploid_refuses_bad_tables_before_it_looks_at_the_context(lib):
    assert _call_diploid_without_context(lib, _call_diploid_tables()) == (INVALID, 0)            # good tables: refused for the missing context only
    for change in (dict(cso=[1, 2, 3]), dict(cso=[0, 3, 2]), dict(sbo=[0, 4, 7, 9]), dict(sbo=[1, 4, 7, 10]), dict(sbo=[0, 4, 4, 10]), dict(end=[100, 90, 50]),
                   dict(beg=[50, 40, 0]), dict(end=[100, 200, -1]), dict(cso=[0, 0, 0], beg=[], end=[], sbo=[0], nbins=0), dict(nchr=-1), dict(csi=[0, 2, 1])):
        assert _call_diploid_without_context(lib, _call_diploid_tables(**change)) == (INVALID, -7), change
    assert lib.canvas_call_diploid(*([None] * 30)) == INVALID


# ---------------------------------------------------------------------------------------------------------------- the executable, wherever no GPU is needed (Program.cs:27-99)
import subprocess

HELP = ["Usage: CanvasDiploidCaller.exe [OPTIONS]+", "Make discrete-valued copy number calls assuming a diploid baseline.", "", "Options:"]


def _exe():
    from canvas_amd import build
    build.build()
    exe = [e for e in build.build_more_tools() if os.path.basename(e) == "CanvasDiploidCaller"]
    assert len(exe) == 1 and os.access(exe[0], os.X_OK)
    return exe[0]


def _run(args):
    r = subprocess.run([_exe()] + args, capture_output=True, text=True, timeout=60)
    lines = r.stdout.splitlines()
    assert lines[0] == ">>>Command-line arguments:"
    return r.returncode, lines[2:], r


def _inputs(tmp_path, genome=True):
    p = tmp_path / "s.partitioned"; p.write_text("")
    v = tmp_path / "s.vaf"; v.write_text("")
    ref = tmp_path / "ref"; ref.mkdir()
    if genome:
        (ref / "GenomeSize.xml").write_text('<sequenceSizes genomeName="t">\n<chromosome fileName="genome.fa" contigName="chr1" totalBases="1000" />\n</sequenceSizes>\n')
    return str(p), str(v), str(ref)


def test_executable_is_built_by_build_more_tools_and_build_tools_is_still_six():
    from canvas_amd import build
    exe = _exe()
    more = build.build_more_tools()
    assert exe in more and os.path.dirname(exe) == os.path.join(build.HERE, "bin") and build.embedded_hash(exe) is not None
    six = build.build_tools()
    assert len(six) == 6 and exe not in six


def test_help_unknown_and_missing_arguments_exit_0(tmp_path):
    p, v, ref = _inputs(tmp_path)
    for args in (["-h"], ["--help"], ["-i", p, "-v", v, "-o", "x", "-r", ref, "-h"]):
        rc, body, _ = _run(args)
        assert rc == 0 and body[:4] == HELP
        for opt in ("-i, --infile=VALUE", "-v, --varfile=VALUE", "-o, --outfile=VALUE", "-r, --reference=VALUE", "-n, --sampleName=VALUE", "-p, --ploidyBed=VALUE", "-d, --dbsnpvcf",
                    "-h, --help", "-s, --qscoreconfig=VALUE", "-t, --truth=VALUE"):
            assert any(opt in l for l in body), opt
    rc, body, _ = _run(["-i", p, "-v", v, "-o", "x", "-r", ref, "--frobnicate"])
    assert rc == 0 and body[0] == "* Error: I don't understand the argument '--frobnicate'" and body[1:5] == HELP
    full = ["-i", p, "-v", v, "-o", str(tmp_path / "o.vcf"), "-r", ref]
    for k in range(0, 8, 2):                                   # each of -i / -v / -o / -r left out in turn
        rc, body, _ = _run(full[:k] + full[k + 2:])
        assert rc == 0 and body[:4] == HELP, full[k]
    assert not (tmp_path / "o.vcf").exists()


def test_missing_files_exit_1_with_the_reference_s_messages(tmp_path):
    p, v, ref = _inputs(tmp_path)
    out = str(tmp_path / "o.vcf")
    rc, body, _ = _run(["-i", p + ".no", "-v", v, "-o", out, "-r", ref])
    assert rc == 1 and body == ["CanvasDiploidCaller.exe: File %s.no does not exist! Exiting." % p]
    rc, body, _ = _run(["-i", p, "-v", v + ".no", "-o", out, "-r", ref])
    assert rc == 1 and body == ["Canvas error: File %s.no does not exist! Exiting." % v]
    os.remove(os.path.join(ref, "GenomeSize.xml"))
    rc, body, _ = _run(["-i", p, "-v", v, "-o", out, "-r", ref])
    assert rc == 1 and body == ["CanvasDiploidCaller.exe: File %s/GenomeSize.xml does not exist! Exiting." % ref]
    assert not os.path.exists(out)


def test_truth_option_exits_1_and_a_missing_qscore_file_too(tmp_path):
    p, v, ref = _inputs(tmp_path)
    rc, body, _ = _run(["-i", p, "-v", v, "-o", str(tmp_path / "o.vcf"), "-r", ref, "-t", "truth.vcf"])
    assert rc == 1 and "not built" in body[0]
    rc, body, _ = _run(["-i", p, "-v", v, "-o", str(tmp_path / "o.vcf"), "-r", ref, "-s", str(tmp_path / "none.json")])
    assert rc == 1 and "does not exist" in body[0]


def test_empty_partitioned_file_needs_no_gpu(tmp_path):
    import diploid_ref as R
    p, v, ref = _inputs(tmp_path)
    out = tmp_path / "o.vcf"
    rc, body, _ = _run(["-i", p, "-v", v, "-o", str(out), "-r", ref, "-n", "S7"])
    assert rc == 0 and body[0] == "CanvasDiploidCaller: No segments loaded; no CNV calls will be made."
    lib = ctypes.CDLL(os.path.join(ROOT, "canvas_amd", "libcanvas_hip.so")); lib.canvas_version.restype = ctypes.c_char_p
    assert out.read_text() == R.files_from_text([], [], [("chr1", 1000)], lib.canvas_version().decode(), ref, "S7")[0]
