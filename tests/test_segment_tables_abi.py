"""CPU-side checks of canvas_segment_tables and canvas_call_diploid_ids: declared, listed, exported and bound with the documented signatures, and every refusal that is
decided on the host arguments comes back with no context at all and *h_nseg untouched (no GPU here: a call that got as far as the device would fail with a HIP error)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("canvas_segment_tables", "canvas_call_diploid_ids")
INVALID = -1
TABLES = "int64_t* h_nseg, int64_t* h_chr_seg_offset, int32_t* h_seg_begin, int32_t* h_seg_end, int64_t* h_seg_bin_offset, int32_t* h_seg_ci4, float* d_count_f32"
BINS = "canvas_ctx* ctx, int64_t nbins, int32_t nchr, const int64_t* h_chr_offset, const int32_t* d_start, const int32_t* d_stop, const int32_t* d_segment_id, const double* d_cov, int64_t cap_seg"


@pytest.fixture(scope="module")
def lib():
    from canvas_amd import build
    so, _ = build.build()
    return ctypes.CDLL(so)


def _declaration(name):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "canvas_hip.h")).read(), flags=re.S)
    m = re.search(r"int32_t\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
    assert m, name
    return re.sub(r"\s+,", ",", re.sub(r"\s+", " ", m.group(1))).strip()


def test_symbols_declared_listed_exported_and_built(lib):
    from canvas_amd import build
    from canvas_amd.lib import ABI_SYMBOLS
    for name in NEW:
        assert name in ABI_SYMBOLS and hasattr(lib, name), name
    assert "segtab.hip" in build.PRODUCT_SRC and os.path.exists(os.path.join(build.CSRC, "segtab.hip"))
    cs = open(os.path.join(ROOT, "hosts", "CanvasHip.cs")).read()
    for name in NEW:
        assert re.search(r"extern int %s\(" % name, cs), name


def test_documented_signatures():
    assert _declaration("canvas_segment_tables") == BINS + ", " + TABLES
    call = _declaration("canvas_call_diploid")
    outputs = call[call.index("double* h_seg_median_count"):]                   # everything canvas_call_diploid returns
    sites = "const int64_t* h_chr_site_offset, const int32_t* d_site_pos, const int32_t* d_site_ref, const int32_t* d_site_alt, const double* h_logistic4"
    assert sites + ", " + outputs in call
    assert _declaration("canvas_call_diploid_ids") == ", ".join((BINS, sites, TABLES, outputs))


def test_python_surface():
    from canvas_amd import Canvas
    assert list(inspect.signature(Canvas.segment_tables).parameters)[:6] == ["self", "chr_offset", "start", "stop", "segment_id", "cov"]
    assert inspect.signature(Canvas.segment_tables).parameters["cov"].default is None
    assert list(inspect.signature(Canvas.call_diploid_ids).parameters)[:10] == ["self", "chr_offset", "start", "stop", "segment_id", "cov", "chr_site_offset", "site_pos", "site_ref", "site_alt"]
    assert list(inspect.signature(Canvas.germline_flow).parameters)[:10] == ["self", "bases", "masks", "hits", "lens", "is_autosome", "chr_site_offset", "site_pos", "site_ref", "site_alt"]


GOOD = dict(nbins=10, nchr=3, off=[0, 4, 4, 10], cap=5)
HOST_REFUSALS = (dict(nbins=0, off=[0, 0, 0, 0]), dict(nbins=-3), dict(cap=-1), dict(off=[1, 4, 4, 10]), dict(off=[0, 5, 4, 10]), dict(off=[0, 4, 4, 9]), dict(off=[0, 4, 4, 11]))


def _tables(lib, entry, ctx=None, **change):
    t = dict(GOOD); t.update(change)
    off = np.array(t["off"], np.int64)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    one = ctypes.c_void_p(64)                                  # stands for a device pointer: never dereferenced on the host
    n = 8
    nseg = ctypes.c_int64(-7)
    tables = [np.zeros(n, np.int64), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n + 1, np.int64), np.zeros(4 * n, np.int32)]
    head = [ctx, ctypes.c_int64(t["nbins"]), ctypes.c_int32(t["nchr"]), P(off), one, one, one, one, ctypes.c_int64(t["cap"])]
    tail = [ctypes.byref(nseg)] + [P(a) for a in tables] + [one]
    if entry == "canvas_segment_tables":
        rc = lib.canvas_segment_tables(*head, *tail)
    else:
        csi = np.zeros(t["nchr"] + 1, np.int64); b4 = np.zeros(4, np.float64)
        f8 = lambda: np.zeros(n + 1, np.float64); i8 = lambda: np.zeros(n + 1, np.int64); i4 = lambda: np.zeros(n + 1, np.int32)
        outs = [f8(), i8(), i4(), f8(), i4(), i4(), f8(), f8(), i4()]; runs = [i8(), i8(), i4(), i4(), f8()]
        nruns = ctypes.c_int64(-7); scal = np.zeros(2, np.float64)
        rc = lib.canvas_call_diploid_ids(*head, P(csi), one, one, one, P(b4), *tail, *[P(a) for a in outs], ctypes.byref(nruns), *[P(a) for a in runs], P(scal), None)
        assert nruns.value == -7
    assert all((a == 0).all() for a in tables)
    return rc, nseg.value


@pytest.mark.parametrize("entry", NEW)
def test_host_decided_refusals_need_no_context(lib, entry):
    assert _tables(lib, entry) == (INVALID, -7)                   # good arguments: refused for the missing context only, *h_nseg is written by the device path alone
    for change in HOST_REFUSALS:
        assert _tables(lib, entry, **change) == (INVALID, -7), change
    assert getattr(lib, entry)(*([None] * (16 if entry == "canvas_segment_tables" else 38))) == INVALID


def test_argument_counts_used_above():
    assert _declaration("canvas_call_diploid_ids").count(",") + 1 == 38 and _declaration("canvas_segment_tables").count(",") + 1 == 16
