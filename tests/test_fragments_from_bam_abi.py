"""canvas_fragments_from_bam on the CPU side: declared in the header, listed in ABI_SYMBOLS, exported by the library, frag.hip among the product's sources, wrapped by
Canvas.fragments_from_bam and declared for the C# hosts; a call without a context is refused."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from canvas_amd import build
    so, _ = build.build()
    return ctypes.CDLL(so)


def test_symbol_is_declared_listed_and_exported(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "canvas_hip.h")).read(), flags=re.S)
    m = re.search(r"int32_t\s+canvas_fragments_from_bam\s*\(([^)]*)\)", hdr)
    assert m, "canvas_fragments_from_bam is not declared in include/canvas_hip.h"
    args = [a.strip() for a in m.group(1).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["ctx", "d_records", "nbytes", "d_record_offsets", "nrecords", "ref_id", "d_bin_start", "d_bin_stop", "nbins",
                                                        "quality_threshold", "d_count", "d_carry", "carry_capacity", "d_state", "h_info"]
    from canvas_amd.lib import ABI_SYMBOLS
    assert "canvas_fragments_from_bam" in ABI_SYMBOLS
    assert hasattr(lib, "canvas_fragments_from_bam")


def test_frag_hip_is_a_product_source():
    from canvas_amd import build
    assert "frag.hip" in build.PRODUCT_SRC and os.path.exists(os.path.join(build.CSRC, "frag.hip"))


def test_wrapper_and_host_declaration_exist():
    from canvas_amd.lib import Canvas
    import inspect
    sig = inspect.signature(Canvas.fragments_from_bam)
    assert list(sig.parameters)[1:] == ["records", "offsets", "ref_id", "bin_start", "bin_stop", "quality_threshold", "counts", "carry", "state", "nbytes", "carry_capacity"]
    assert sig.parameters["quality_threshold"].default == 3 and sig.parameters["carry_capacity"].default is None
    cs = open(os.path.join(ROOT, "hosts", "CanvasHip.cs")).read()
    assert re.search(r"extern int canvas_fragments_from_bam\(IntPtr ctx,", cs)


def test_call_without_a_context_is_invalid(lib):
    fn = lib.canvas_fragments_from_bam
    fn.restype = ctypes.c_int32
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                   ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    assert fn(None, None, 0, None, 0, 0, None, None, 0, 3, None, None, 0, None, None) == -1            # CANVAS_ERR_INVALID
