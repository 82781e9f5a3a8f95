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


def test_a_touched_or_new_tool_header_makes_every_tool_stale(tmp_path, monkeypatch):
    """build_tools() hashes every *.hpp of canvas_amd/tools: after a header changed, or a new one appeared, all six tools are compiled again with another embedded
    hash; with nothing changed none is.  (The compiler is replaced by a stand-in that writes the hash marker a real binary carries: this is about staleness.)"""
    import shutil
    from canvas_amd import build
    here = tmp_path / "canvas_amd"
    shutil.copytree(os.path.join(build.HERE, "tools"), here / "tools")
    monkeypatch.setattr(build, "HERE", str(here))
    compiled = []

    def stand_in(cmd):
        out = cmd[cmd.index("-o") + 1]
        define = [a for a in cmd if a.startswith("-DCANVAS_SRC_HASH=")][0]
        open(out, "wb").write(build.HASH_MARKER + define.split("=", 1)[1].strip('"').encode())
        compiled.append(out)
    monkeypatch.setattr(build.subprocess, "check_call", stand_in)

    def hashes():
        compiled.clear()
        outs = build.build_tools()
        assert len(outs) == 6
        return [build.embedded_hash(o) for o in outs], len(compiled)
    first, n = hashes()
    assert n == 6 and len(set(first)) == 6
    assert hashes() == (first, 0)
    with open(here / "tools" / "bam_io.hpp", "a") as f:
        f.write("// touched\n")
    second, n = hashes()
    assert n == 6 and all(a != b for a, b in zip(first, second))
    (here / "tools" / "a_new_header.hpp").write_text("#pragma once\n")
    third, n = hashes()
    assert n == 6 and all(a != b for a, b in zip(second, third))
