"""canvas_bam_frame at the C ABI, without a GPU: the rule's layout, the codes of the header against those of canvas_amd.lib and tests/frame_ref.py, and the one
refusal that can be made without a device: a NULL context, whatever else is passed, follows no pointer.  The other CANVAS_ERR_INVALID cases need a live context to
be told apart from that one; tests/test_bam_frame_gpu.py::test_refusals_with_a_live_context makes each of them and checks that no buffer was written."""
import ctypes
import os
import re

import numpy as np
import pytest

import frame_ref as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from canvas_amd import build
    so, _ = build.build()
    lib = ctypes.CDLL(so)
    lib.canvas_bam_frame.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    lib.canvas_bam_frame.restype = ctypes.c_int32
    return lib


def test_rule_is_16_bytes():
    from canvas_amd.lib import BAM_FRAME_RULE
    import canvas_amd
    assert BAM_FRAME_RULE.itemsize == 16 and canvas_amd.BAM_FRAME_RULE is BAM_FRAME_RULE
    assert [BAM_FRAME_RULE.fields[n][1] for n in ("kind", "ref_id", "paired_end", "sorted")] == [0, 4, 8, 12]
    assert all(BAM_FRAME_RULE.fields[n][0] == np.dtype("<i4") for n in BAM_FRAME_RULE.names)
    hdr = open(os.path.join(ROOT, "include", "canvas_hip.h")).read()
    assert re.search(r"typedef struct \{ int32_t kind; int32_t ref_id; int32_t paired_end; int32_t sorted; \} canvas_bam_frame_rule;", hdr)
    src = open(os.path.join(ROOT, "canvas_amd", "csrc", "bam_frame.hpp")).read()
    assert re.search(r"struct BamFrameRule \{ int32_t kind, ref_id, paired_end, sorted; \};", src)


def test_codes_of_the_header():
    from canvas_amd import lib as L
    hdr = open(os.path.join(ROOT, "include", "canvas_hip.h")).read()
    codes = dict((n, int(v)) for n, v in re.findall(r"#define (CANVAS_BAM_FRAME_\w+) (\d+)", hdr))
    assert codes == dict(CANVAS_BAM_FRAME_ALL=0, CANVAS_BAM_FRAME_SNV=1, CANVAS_BAM_FRAME_HITS=2, CANVAS_BAM_FRAME_FRAGMENTS=3, CANVAS_BAM_FRAME_NONE=0,
                         CANVAS_BAM_FRAME_STOPPED=1, CANVAS_BAM_FRAME_MALFORMED=2, CANVAS_BAM_FRAME_UNSORTED=3, CANVAS_BAM_FRAME_CAPACITY=4)
    for name, value in codes.items():
        assert getattr(L, name[len("CANVAS_"):]) == value, name
    assert [FR.ALL, FR.SNV, FR.HITS, FR.FRAGMENTS] == [L.BAM_FRAME_ALL, L.BAM_FRAME_SNV, L.BAM_FRAME_HITS, L.BAM_FRAME_FRAGMENTS]
    assert [FR.NONE, FR.STOPPED, FR.EV_MALFORMED, FR.EV_UNSORTED, FR.CAPACITY] == [L.BAM_FRAME_NONE, L.BAM_FRAME_STOPPED, L.BAM_FRAME_MALFORMED, L.BAM_FRAME_UNSORTED, L.BAM_FRAME_CAPACITY]
    # the classes and kinds of the shared header, by name
    src = open(os.path.join(ROOT, "canvas_amd", "csrc", "bam_frame.hpp")).read()
    enums = dict((n, int(v)) for n, v in re.findall(r"\b(BAM_FRAME_\w+) = (\d+)", src))
    assert [enums["BAM_FRAME_" + n] for n in ("TAKE", "SKIP", "TAKE_AND_STOP", "STOP", "MALFORMED", "UNSORTED")] == [FR.TAKE, FR.SKIP, FR.TAKE_AND_STOP, FR.STOP, FR.MALFORMED, FR.UNSORTED]
    assert [enums["BAM_FRAME_" + n] for n in ("ALL", "SNV", "HITS", "FRAGMENTS")] == [0, 1, 2, 3]


def test_refused_without_a_context(lib):
    """no context: CANVAS_ERR_INVALID whatever else is passed, and none of the pointers is followed (they point nowhere)"""
    rule = np.zeros(1, [("kind", "<i4"), ("ref_id", "<i4"), ("paired_end", "<i4"), ("sorted", "<i4")])
    info = np.full(8, -7, np.int64)
    nowhere = ctypes.c_void_p(8)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    for args in ((nowhere, 100, 0, p(rule), nowhere, 10, nowhere, p(info)), (None, 0, 0, None, None, 0, None, None), (nowhere, 100, 101, nowhere, nowhere, -1, nowhere, nowhere)):
        assert lib.canvas_bam_frame(None, *args) == -1      # CANVAS_ERR_INVALID
    assert (info == -7).all()
