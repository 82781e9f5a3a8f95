"""canvas_amd/bin/CanvasSmooth end to end: a gzip .cleaned file goes in, and the output must be, byte for byte, the lines the CPU restatement (tests/smooth_ref.py)
and the F2 format imply — the bins CanvasSmooth drops and the chromosome that vanishes included."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import smooth_ref as R
from gpu_common import get_canvas

pytestmark = pytest.mark.gpu
EXE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "canvas_amd", "bin", "CanvasSmooth")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    get_canvas().close()


def _run(args):
    return subprocess.run([EXE] + args, capture_output=True, text=True, timeout=300)


def _rows(spec, seed):
    """spec: [(name, bins)] in file order -> [(name, start, stop, count text, gc)]"""
    rng = np.random.RandomState(seed)
    rows, at = [], {}
    for name, n in spec:
        for _ in range(n):
            s = at.get(name, 1000)
            at[name] = s + 100 + int(rng.randint(0, 50))
            rows.append((name, s, at[name], "%.2f" % (rng.randint(8000, 8060) / 100.0 if rng.rand() > 0.02 else rng.uniform(0, 4000)), int(rng.randint(20, 70))))
    return rows


def _write(path, rows):
    with gzip.open(path, "wb") as f:
        for r in rows:
            f.write(("%s\t%d\t%d\t%s\t%d\n" % r).encode())


def _expected(rows, W):
    names = []
    for r in rows:
        if r[0] not in names:
            names.append(r[0])
    out = []
    for name in names:                                    # grouped by name in order of first appearance, stably
        mine = [r for r in rows if r[0] == name]
        sm = R.smooth_windows(np.array([np.float32(float(r[3])) for r in mine], np.float32), W)
        for r, c in zip(mine, sm):                        # Enumerable.Zip: the bins beyond the smoothed counts are dropped
            out.append("%s\t%d\t%d\t%s\t%d\n" % (r[0], r[1], r[2], O.format_f2(float(c)), r[4]))
    return "".join(out).encode()


def test_tool_end_to_end(tmp_path):
    rows = _rows([("chr1", 9000), ("chrSmall", 4), ("chrOne", 1)], 1)
    src = str(tmp_path / "s.cleaned"); _write(src, rows)
    for W in (0, 2, 3):
        out = str(tmp_path / ("s.w%d.smoothed" % W))
        r = _run(["-i", src, "-o", out] + (["-w", str(W)] if W else []))
        assert r.returncode == 0, r.stderr
        got = gzip.open(out, "rb").read()
        assert got == _expected(rows, W), W
        left = [sum(line.startswith(name + b"\t") for line in got.splitlines()) for name in (b"chr1", b"chrSmall", b"chrOne")]
        assert left == {0: [9000, 4, 1], 2: [9000, 3, 0], 3: [9000, 0, 0]}[W] == [R.out_len(n, W) for n in (9000, 4, 1)]      # dropped bins, vanished chromosomes
        assert "Launch smoothing jobs..." in r.stdout and "Completed smoothing jobs." in r.stdout


def test_a_name_that_reappears_joins_its_first_run(tmp_path):
    rows = _rows([("chrA", 50), ("chrB", 30), ("chrA", 40), ("chrC", 3), ("chrB", 5)], 2)
    src = str(tmp_path / "r.cleaned"); _write(src, rows)
    out = str(tmp_path / "r.smoothed")
    r = _run(["--infile=" + src, "--outfile", out, "--maxHalfWindowSize", "2"])
    assert r.returncode == 0, r.stderr
    got = gzip.open(out, "rb").read()
    assert got == _expected(rows, 2)
    assert [R.out_len(n, 2) for n in (90, 35, 3)] == [90, 35, 1]                 # 3 bins: 3 after h = 1, max(0, 3-2) + max(0, 3-2-1) = 1 after h = 2
    assert [l.split(b"\t")[0] for l in got.splitlines()] == [b"chrA"] * 90 + [b"chrB"] * 35 + [b"chrC"] * 1


def test_unsorted_bins_exit_1(tmp_path):
    rows = _rows([("chrA", 20), ("chrB", 20)], 3)
    rows[30], rows[31] = rows[31], rows[30]               # inside chrB
    src = str(tmp_path / "u.cleaned"); _write(src, rows)
    out = tmp_path / "u.smoothed"
    r = _run(["-i", src, "-o", str(out), "-w", "1"])
    assert r.returncode == 1 and not out.exists()
    assert "Bins are not sorted in ascending order by the start position. First offending bin: chrB\t%d\t%d" % (rows[31][1], rows[31][2]) in r.stderr
    # the check compares with the previous LINE unless the name is new (IO.cs:64-78): a run of chrA that comes back behind chrB with smaller starts trips it,
    # a chromosome that is new never does
    rows = _rows([("chrA", 5), ("chrB", 12), ("chrA", 5)], 4)
    src2 = str(tmp_path / "v.cleaned"); _write(src2, rows)
    r = _run(["-i", src2, "-o", str(out), "-w", "1"])
    back = rows[17]
    assert back[0] == "chrA" and back[1] > rows[4][1] and back[1] < rows[16][1]                       # sorted within chrA, yet behind chrB's last start
    assert r.returncode == 1 and "First offending bin: chrA\t%d\t%d" % (back[1], back[2]) in r.stderr
