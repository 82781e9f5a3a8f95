"""CPU-side checks of the FlagUniqueKmers surface: the two entry points are declared, listed and exported, the executable is built, and without arguments it
prints the reference's usage lines and exits 0 (Tools/FlagUniqueKmers/Program.cs:13-18) — no GPU needed for any of it."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("canvas_flag_unique_kmers", "canvas_fasta_case_from_mask")


def test_symbols_declared_listed_and_exported():
    from canvas_amd import build
    from canvas_amd.lib import ABI_SYMBOLS
    so, _ = build.build()
    lib = ctypes.CDLL(so)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "canvas_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(canvas_\w+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in ABI_SYMBOLS and hasattr(lib, name), name
    assert "kmer.hip" in build.PRODUCT_SRC
    # no context: CANVAS_ERR_INVALID, nothing touched
    assert lib.canvas_flag_unique_kmers(None, 0, None, None, None, ctypes.c_int64(0), None) == -1
    assert lib.canvas_fasta_case_from_mask(None, None, ctypes.c_int64(0), None) == -1


def test_python_surface():
    from canvas_amd import Canvas
    assert callable(Canvas.flag_unique_kmers) and callable(Canvas.fasta_case_from_mask)


def test_executable_is_built_and_prints_usage():
    from canvas_amd import build
    build.build()
    exe = [e for e in build.build_tools() if os.path.basename(e) == "FlagUniqueKmers"]
    assert len(exe) == 1 and os.access(exe[0], os.X_OK)
    for args in ([], ["only_one_argument.fa"]):
        r = subprocess.run([exe[0]] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 0
        assert r.stderr.splitlines() == ["Usage info:", "  FlagUniqueKmers $InputFASTA $OutputFASTA"]
        assert r.stdout == ""
    assert not os.path.exists("only_one_argument.fa")


def test_missing_input_exits_1(tmp_path):
    """the input is opened before the GPU context is asked for"""
    from canvas_amd import build
    build.build()
    exe = os.path.join(build.HERE, "bin", "FlagUniqueKmers")
    out = tmp_path / "out.fa"
    r = subprocess.run([exe, str(tmp_path / "missing.fa"), str(out)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "cannot read" in r.stderr
    assert not out.exists()
