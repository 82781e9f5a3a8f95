"""CPU-side checks of canvas_call_somatic: the entry is declared, listed, built and exported, the header, canvas_amd/lib.py and hosts/CanvasHip.cs lay its three structs out
alike (sizes and offsets computed from the header's own declarations), and the entry refuses bad arguments before it looks at the context (no GPU here: a call that got as
far as the device would fail with a HIP error instead)."""
import ctypes
import os
import re

import numpy as np
import pytest

import somatic_call_cases as C
import somatic_call_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
STRUCTS = {"canvas_somatic_call_params": "SomaticCallParams", "canvas_somatic_call_out": "SomaticCallOut", "canvas_somatic_call_scalars": "SomaticCallScalars"}
SCALARS = {"int32_t": (4, ctypes.c_int32), "uint32_t": (4, ctypes.c_uint32), "int64_t": (8, ctypes.c_int64), "float": (4, ctypes.c_float), "double": (8, ctypes.c_double)}
CS_TYPES = {"int": "int32_t", "uint": "uint32_t", "long": "int64_t", "float": "float", "double": "double", "IntPtr": "*"}


@pytest.fixture(scope="module")
def lib():
    from canvas_amd import build
    so, _ = build.build()
    lib = ctypes.CDLL(so)
    lib.canvas_call_somatic.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int32] + [ctypes.c_void_p] * 16
    return lib


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "canvas_hip.h")).read(), flags=re.S)


def _header_fields(name):
    """[(field, C type)] of `typedef struct name { ... } name;`, pointers as 'T*', an embedded struct under its own name"""
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
            out.append((f.lstrip("* "), ctype.rstrip("*") + ("*" if star else "")))
    return out


def _layout(name):
    """offsets and size by the C rules (natural alignment), from the header alone"""
    off, align_max, offsets = 0, 1, {}
    for fname, ctype in _header_fields(name):
        if ctype.endswith("*"):
            size = align = 8
        elif ctype in SCALARS:
            size = align = SCALARS[ctype][0]
        else:
            _, size, align = _layout(ctype)
        off = (off + align - 1) // align * align
        offsets[fname] = off
        off += size
        align_max = max(align_max, align)
    return offsets, (off + align_max - 1) // align_max * align_max, align_max


def test_symbol_declared_listed_built_and_exported(lib):
    from canvas_amd import build, Canvas
    from canvas_amd.lib import ABI_SYMBOLS
    assert "canvas_call_somatic" in set(re.findall(r"\b(canvas_\w+)\s*\(", _header()))
    assert "canvas_call_somatic" in ABI_SYMBOLS and hasattr(lib, "canvas_call_somatic") and callable(Canvas.call_somatic)
    assert "call.hip" in build.PRODUCT_SRC and "somatic.hip" in build.PRODUCT_SRC
    src = open(os.path.join(build.CSRC, "call.hip")).read()
    assert 'extern "C" int32_t canvas_call_somatic(' in src and "k_scall_assign" in src and "k_scall_mean" in src and "k_scall_compact" in src
    for f in ("call.hip", "somatic.hip"):                      # the model points' host code is shared, not copied
        assert '#include "somatic_points.hpp"' in open(os.path.join(build.CSRC, f)).read()
    cs = open(os.path.join(ROOT, "hosts", "CanvasHip.cs")).read()
    assert re.search(r"extern int canvas_call_somatic\(", cs)
    assert len(re.search(r"extern int canvas_call_somatic\((.*?)\);", cs, flags=re.S).group(1).split(",")) == 20
    assert len(re.search(r"int32_t canvas_call_somatic\((.*?)\);", _header(), flags=re.S).group(1).split(",")) == 20


def test_constants_and_defaults():
    from canvas_amd import lib as L
    h = _header()
    define = lambda n: int(re.search(r"#define %s \(?(-?\d+)u?\)?" % n, h).group(1))
    assert L.ERR_SOMATIC_FEW_SEGMENTS == define("CANVAS_ERR_SOMATIC_FEW_SEGMENTS") == -8
    assert (L.SOMATIC_MEAN_NONE, L.SOMATIC_MEAN_WALK, L.SOMATIC_MEAN_EXACT) == (define("CANVAS_SOMATIC_MEAN_NONE"), define("CANVAS_SOMATIC_MEAN_WALK"), define("CANVAS_SOMATIC_MEAN_EXACT")) == (-1, 0, 1)
    assert sorted(L.SOMATIC_CALL_DEFAULTS) == sorted(CR.CALL_DEFAULTS)
    for k, v in CR.CALL_DEFAULTS.items():
        assert L.SOMATIC_CALL_DEFAULTS[k] == v or (v != v and L.SOMATIC_CALL_DEFAULTS[k] != L.SOMATIC_CALL_DEFAULTS[k]), k
    d = L.SOMATIC_CALL_DEFAULTS                                                  # SomaticCallerParameters.json, QualityScoreParameters.cs:9-12, SomaticCaller.cs:70
    assert (d["minimum_variant_frequencies"], d["minimum_call_size"], d["quality_filter_threshold"], d["merge_span"]) == (50, 50000, 10, 1)
    assert (d["coverage_weighting"], d["coverage_weighting_with_maf_segmentation"], d["evenness_score_threshold"], d["min_evenness_score"]) == (0.333, 0.20, 94.5, 88.0)
    assert (d["lower_coverage_level_weighting_factor"], d["upper_coverage_level_weighting_factor"]) == (4.0, 2.355)
    assert (d["logistic_intercept"], d["logistic_log_bin_count"], d["logistic_model_distance"], d["logistic_distance_ratio"]) == (-0.5143, 0.8596, -50.4366, -0.6511)
    cs = open(os.path.join(ROOT, "hosts", "CanvasHip.cs")).read()
    assert "ErrSomaticFewSegments = -8, SomaticMeanNone = -1, SomaticMeanWalk = 0, SomaticMeanExact = 1" in cs


@pytest.mark.parametrize("name", sorted(STRUCTS))
def test_struct_layout_is_the_same_in_header_python_and_csharp(name):
    from canvas_amd import lib as L
    hdr = _header_fields(name)
    offsets, size, _ = _layout(name)
    py = getattr(L, STRUCTS[name])
    assert [f[0] for f in py._fields_] == [f[0] for f in hdr]
    assert ctypes.sizeof(py) == size
    for (fname, ftype), (_, ctype) in zip(py._fields_, hdr):
        assert getattr(py, fname).offset == offsets[fname], fname
        want = ctypes.c_void_p if ctype.endswith("*") else SCALARS[ctype][1] if ctype in SCALARS else L.SomaticParams
        assert ftype is want, fname
    cs = open(os.path.join(ROOT, "hosts", "CanvasHip.cs")).read()
    assert re.search(r"\[StructLayout\(LayoutKind\.Sequential\)\] public struct %s\b" % name, cs)
    body = re.search(r"struct %s\s*\{(.*?)\n        \}" % name, cs, flags=re.S).group(1)
    got = []
    for decl in body.split(";"):
        m = re.match(r"\s*public (\w+) (.*)$", decl.strip(), flags=re.S)
        if m:
            for f in m.group(2).split(","):
                got.append((f.strip(), CS_TYPES.get(m.group(1), m.group(1))))
    assert [g[0] for g in got] == [f[0] for f in hdr]
    for (fname, cstype), (_, ctype) in zip(got, hdr):
        assert (ctype.endswith("*") if cstype == "*" else cstype == ctype), fname
    if name == "canvas_somatic_call_params":
        assert offsets["minimum_variant_frequencies"] == ctypes.sizeof(L.SomaticParams) == 56 and offsets["coverage_weighting"] == 96 and size == 192
    if name == "canvas_somatic_call_out":
        assert [f for f, _, _ in L.SOMATIC_CALL_OUT] == [f[0] for f in hdr]
        want = {"double*": np.float64, "int32_t*": np.int32, "int64_t*": np.int64}
        assert [dt for _, dt, _ in L.SOMATIC_CALL_OUT] == [want[f[1]] for f in hdr]


def _call(lib, case, ctx=None, nulls=(), out_null=None, **changes):
    """canvas_call_somatic with host tables of `case`, device pointers that are never followed (the context is NULL) and scalars preset to 7s"""
    from canvas_amd import lib as L
    c = dict(case, **{k: v for k, v in changes.items() if k in case})
    cso, csi = np.ascontiguousarray(c["chr_seg_offset"], np.int64), np.ascontiguousarray(c["chr_site_offset"], np.int64)
    beg, end, sbo = np.ascontiguousarray(c["seg_begin"], np.int32), np.ascontiguousarray(c["seg_end"], np.int32), np.ascontiguousarray(c["seg_bin_offset"], np.int64)
    ref = np.ascontiguousarray(c["seg_ref_cn"], np.int32)
    nseg = len(beg)
    params = dict(c["params"], **changes.get("params", {}))
    fitp = L.SomaticParams(**dict(L.SOMATIC_DEFAULTS, **{k: v for k, v in params.items() if k in L.SOMATIC_DEFAULTS}))
    cp = L.SomaticCallParams(fit=fitp, **dict(L.SOMATIC_CALL_DEFAULTS, genome_length=changes.get("genome_length", c["genome_length"]), **{k: v for k, v in params.items() if k in L.SOMATIC_CALL_DEFAULTS}))
    arrays = {n: np.zeros(nseg + 2, dt) for n, dt, _ in L.SOMATIC_CALL_OUT}
    co = L.SomaticCallOut(*[None if n == out_null else arrays[n].ctypes.data for n, _, _ in L.SOMATIC_CALL_OUT])
    sc = L.SomaticCallScalars(); sc.nruns = 7; sc.stages = 7
    res = L.SomaticResult(); res.nmodels = 7
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    fake = ctypes.c_void_p(4096)                                 # stands for a device array: never read on the host
    eo = es = ee = None
    if "excluded" in c:
        eo = np.concatenate([[0], np.cumsum([len(e[0]) for e in c["excluded"]])]).astype(np.int64)
        es = np.ascontiguousarray(np.concatenate([e[0] for e in c["excluded"]] + [np.zeros(1, np.int32)]), np.int32)
        ee = np.ascontiguousarray(np.concatenate([e[1] for e in c["excluded"]] + [np.zeros(1, np.int32)]), np.int32)
    args = [ctx, len(c["counts"]) if "nbins" not in changes else changes["nbins"], fake, len(cso) - 1, P(cso), P(beg), P(end), P(sbo), P(csi), fake, fake, fake, P(ref),
            None if eo is None else P(eo), None if es is None else P(es), None if ee is None else P(ee), ctypes.byref(cp), ctypes.byref(co), ctypes.byref(sc), ctypes.byref(res)]
    for k in nulls:
        args[k] = None
    return lib.canvas_call_somatic(*args), sc.nruns, sc.stages, res.nmodels


def test_refuses_bad_arguments_before_it_looks_at_the_context(lib):
    """the host tables and parameters are checked first: with no context at all, the scalars and the fit's result are cleared exactly when they have passed"""
    good = C.built("merges")
    untouched, cleared = (INVALID, 7, 7, 7), (INVALID, 0, 0, 0)
    assert _call(lib, good) == cleared                                        # refused for the missing context only
    assert _call(lib, good, nulls=(12,)) == cleared                           # no reference copy numbers: 2 everywhere
    assert _call(lib, good, nulls=(13, 14, 15)) == cleared                    # no excluded intervals
    for k in (4, 5, 6, 7, 8, 16, 17, 18, 19, 2, 9, 10, 11, 14, 15):           # a NULL table, device array, parameter struct, output struct, scalars or result
        assert _call(lib, good, nulls=(k,))[0] == INVALID and (k in (18, 19) or _call(lib, good, nulls=(k,)) == untouched), k
    assert _call(lib, good, out_null="seg_run") == untouched and _call(lib, good, out_null="run_filter") == untouched

    def changed(key, index, value):
        a = good[key].copy(); a[index] = value
        return _call(lib, good, **{key: a})
    assert changed("chr_seg_offset", 0, 1) == untouched and changed("chr_site_offset", 1, -1) == untouched
    assert changed("chr_seg_offset", 1, good["chr_seg_offset"][2] + 1) == untouched
    assert changed("seg_bin_offset", 0, 1) == untouched and changed("seg_bin_offset", 4, good["seg_bin_offset"][3]) == untouched
    assert _call(lib, good, nbins=len(good["counts"]) + 1) == untouched and _call(lib, good, nbins=-1) == untouched
    assert changed("seg_end", 3, good["seg_begin"][3] - 1) == untouched
    assert changed("seg_begin", 3, good["seg_begin"][2] - 1) == untouched and changed("seg_end", 3, good["seg_end"][2]) == untouched
    ex = [(e[0].copy(), e[1].copy()) for e in good["excluded"]]
    ex[0][0][1] = ex[0][0][0] - 1
    assert _call(lib, dict(good, excluded=ex)) == untouched                   # excluded intervals out of order
    for p in (dict(maximum_copy_number=1), dict(maximum_copy_number=11), dict(lower_coverage_level_weighting_factor=0.0), dict(upper_coverage_level_weighting_factor=float("inf")),
              dict(coverage_weighting=float("nan")), dict(logistic_model_distance=float("inf")), dict(user_ploidy=0.0), dict(user_purity=1.5), dict(user_purity=float("nan"))):
        assert _call(lib, good, params=p) == untouched, p
    assert _call(lib, good, genome_length=0) == untouched
    none = dict(good, chr_seg_offset=np.zeros(len(good["chr_seg_offset"]), np.int64))
    assert _call(lib, none)[1:] == (7, 7, 7)                                  # no segments
    for name in ("base", "merges enrichment", "high copy number"):
        assert _call(lib, C.built(name)) == cleared, name
