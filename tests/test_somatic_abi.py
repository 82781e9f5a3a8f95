"""CPU-side checks of the CanvasSomaticCaller surface: canvas_somatic_model_fit is declared, listed, built and exported, the header, canvas_amd/lib.py and hosts/CanvasHip.cs
lay the four structs out alike, and the entry refuses bad arguments before it touches the device (no GPU here: a call that got as far as the device would fail with a HIP
error instead)."""
import ctypes
import os
import re

import numpy as np
import pytest

import somatic_cases as Cs
import somatic_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, CAPACITY = -1, -4
STRUCTS = ("canvas_somatic_params", "canvas_somatic_grid", "canvas_somatic_result", "canvas_somatic_models")
C_TYPES = {"int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double,
           "int32_t*": ctypes.c_void_p, "double*": ctypes.c_void_p}
CS_TYPES = {"int": "int32_t", "uint": "uint32_t", "long": "int64_t", "float": "float", "double": "double", "IntPtr": "*"}


@pytest.fixture(scope="module")
def lib():
    from canvas_amd import build
    so, _ = build.build()
    lib = ctypes.CDLL(so)
    lib.canvas_somatic_model_fit.argtypes = [ctypes.c_void_p, ctypes.c_int64] + [ctypes.c_void_p] * 4 + [ctypes.c_int32] + [ctypes.c_void_p] * 6
    return lib


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "canvas_hip.h")).read(), flags=re.S)


def _header_fields(name):
    """[(field, C type, array length or 0)] of `typedef struct name { ... } name;`"""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), _header(), flags=re.S).group(1)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, rest = decl.split(None, 1)
        for f in rest.split(","):
            f = f.strip()
            star = f.startswith("*") or ctype.endswith("*")
            m = re.match(r"\*?\s*(\w+)(?:\[(.*?)\])?$", f)
            n = m.group(2)
            out.append((m.group(1), ctype.rstrip("*") + ("*" if star else ""), 0 if n is None else 11 if "CANVAS_SOMATIC_MAX_CN" in n else int(n)))
    return out


def test_symbol_declared_listed_built_and_exported(lib):
    from canvas_amd import build
    from canvas_amd.lib import ABI_SYMBOLS
    assert "canvas_somatic_model_fit" in set(re.findall(r"\b(canvas_\w+)\s*\(", _header()))
    assert "canvas_somatic_model_fit" in ABI_SYMBOLS and hasattr(lib, "canvas_somatic_model_fit")
    assert "somatic.hip" in build.PRODUCT_SRC and os.path.exists(os.path.join(build.CSRC, "somatic.hip"))
    cs = open(os.path.join(ROOT, "hosts", "CanvasHip.cs")).read()
    assert re.search(r"extern int canvas_somatic_model_fit\(", cs)


def test_python_surface_and_constants():
    from canvas_amd import Canvas, lib as L
    assert callable(Canvas.somatic_model_fit)
    h = _header()
    define = lambda n: int(re.search(r"#define %s \(?(-?\d+)u?\)?" % n, h).group(1))
    assert L.SOMATIC_TILE == define("CANVAS_SOMATIC_TILE") == Cs.TILE and L.SOMATIC_MAX_CN == define("CANVAS_SOMATIC_MAX_CN")
    assert (L.ERR_SOMATIC_NO_MODEL, L.ERR_SOMATIC_NO_SCORE) == (define("CANVAS_ERR_SOMATIC_NO_MODEL"), define("CANVAS_ERR_SOMATIC_NO_SCORE")) == (-6, -7)
    assert (L.SOMATIC_INFO_CLUSTER_TERM, L.SOMATIC_INFO_INDEX_CUTOFF) == (define("CANVAS_SOMATIC_INFO_CLUSTER_TERM"), define("CANVAS_SOMATIC_INFO_INDEX_CUTOFF")) == (R.INFO_CLUSTER_TERM, R.INFO_INDEX_CUTOFF)
    assert (L.SOMATIC_MODEL_VALID, L.SOMATIC_MODEL_SCORED) == (define("CANVAS_SOMATIC_MODEL_VALID"), define("CANVAS_SOMATIC_MODEL_SCORED")) == (R.VALID, R.SCORED)
    assert L.SOMATIC_DEFAULTS == R.DEFAULTS                                  # SomaticCallerParameters.json
    cs = open(os.path.join(ROOT, "hosts", "CanvasHip.cs")).read()
    assert "ErrSomaticNoModel = -6, ErrSomaticNoScore = -7, SomaticTile = 256, SomaticMaxCn = 10" in cs
    src = open(os.path.join(ROOT, "canvas_amd", "csrc", "somatic.hip")).read()
    assert re.search(r"#define SOM_T %d\b" % L.SOMATIC_TILE, src)


@pytest.mark.parametrize("name", STRUCTS)
def test_struct_layout_is_the_same_in_header_python_and_csharp(name):
    from canvas_amd import lib as L
    hdr = _header_fields(name)
    py = getattr(L, {"canvas_somatic_params": "SomaticParams", "canvas_somatic_grid": "SomaticGrid", "canvas_somatic_result": "SomaticResult", "canvas_somatic_models": "SomaticModels"}[name])
    assert [f[0] for f in py._fields_] == [f[0] for f in hdr]
    for (fname, ftype), (_, ctype, n) in zip(py._fields_, hdr):
        assert ftype == (C_TYPES[ctype] * n if n else C_TYPES[ctype]), fname
    cs = open(os.path.join(ROOT, "hosts", "CanvasHip.cs")).read()
    body = re.search(r"struct %s\s*\{(.*?)\n        \}" % name, cs, flags=re.S).group(1)
    got = []
    for decl in body.split(";"):
        m = re.match(r"\s*public (fixed )?(\w+) (.*)$", decl.strip(), flags=re.S)
        if m:
            for f in m.group(3).split(","):
                fm = re.match(r"(\w+)(?:\[(\d+)\])?$", f.strip())
                got.append((fm.group(1), CS_TYPES[m.group(2)], int(fm.group(2) or 0)))
    assert [g[0] for g in got] == [f[0] for f in hdr]
    for (fname, cstype, n), (_, ctype, hn) in zip(got, hdr):
        assert (ctype.endswith("*") if cstype == "*" else cstype == ctype) and n == hn, fname


def _call(lib, c, capacity=None, nulls=()):
    from canvas_amd import lib as L
    a = [np.ascontiguousarray(c[k], dt) for k, dt in (("coverage", np.float64), ("maf", np.float64), ("weight", np.float64), ("length", np.int32))]
    grid = L.SomaticGrid(c["min_coverage"], c["max_coverage"], c["hard_limit"], c["fixed_percent_purity"], c["fixed_coverage"], int(c["is_enrichment"]), c["mmac"], c["cwf"], c["genome_length"])
    sp = L.SomaticParams(**dict(L.SOMATIC_DEFAULTS, **c["params"]))
    res = L.SomaticResult(); res.nmodels = -7
    sm = L.SomaticModels(capacity, *([None] * 11)) if capacity is not None else None
    P = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    args = [None, len(a[0]), P(a[0]), P(a[1]), P(a[2]), P(a[3]), 0, ctypes.byref(grid), ctypes.byref(sp), ctypes.byref(res), None, None, ctypes.byref(sm) if sm is not None else None]
    for k in nulls:
        args[k] = None
    return lib.canvas_somatic_model_fit(*args), res.nmodels


def test_refuses_bad_arguments_before_it_looks_at_the_context(lib):
    """host inputs are checked first: with no context at all, result.nmodels is written exactly when they have passed"""
    good = Cs.built("size 64")
    assert _call(lib, good) == (INVALID, 15)                                 # refused for the missing context only
    assert _call(lib, Cs.built("mmac")) == (INVALID, len(R.grid_of(Cs.built("mmac"))))
    for name, c in Cs.invalid_cases().items():
        assert _call(lib, c) == (INVALID, -7), name
    for change in (dict(genome_length=0), dict(hard_limit=100), dict(hard_limit=-1), dict(fixed_percent_purity=101), dict(min_coverage=0), dict(max_coverage=100001),
                   dict(mmac=float("nan")), dict(cwf=float("inf")), dict(params=dict(maximum_related_models=0)), dict(params=dict(deviation_index_cutoff=-1))):
        assert _call(lib, dict(good, **change)) == (INVALID, -7), change
    for k, v in (("coverage", np.inf), ("weight", np.nan), ("maf", np.nan)):
        c = dict(good, **{k: good[k].copy()}); c[k][7] = v
        assert _call(lib, c) == (INVALID, -7), k
    c = dict(good, length=good["length"].copy()); c["length"][0] = -1
    assert _call(lib, c) == (INVALID, -7)
    for k in (2, 3, 4, 5, 7, 8, 9):                                           # a NULL array, grid, parameter struct or result
        assert _call(lib, good, nulls=(k,))[0] == INVALID
    assert _call(lib, good, capacity=14) == (CAPACITY, -7) and _call(lib, good, capacity=15) == (INVALID, 15)


def test_grid_of_lib_matches_the_restatement():
    from canvas_amd.lib import somatic_grid
    for name in ("size 64", "mmac", "purity 5", "fixed", "float purity 57", "coverage 10"):
        c = Cs.built(name)
        assert somatic_grid(c["min_coverage"], c["max_coverage"], c["hard_limit"], c["mmac"], c["fixed_percent_purity"], c["fixed_coverage"]) == R.grid_of(c), name
