"""CPU-side checks of the partition-state entries: canvas_partition_states_cbs / _breakpoints, canvas_reference_copy_numbers and canvas_call_somatic_ids are declared,
listed, exported and bound; the Python surface is there; the breakpoints entry refuses bad arguments before it looks at the context (no GPU here: a call that got as far as
the device would fail with a HIP error instead); and canvas_reference_copy_numbers, which needs no GPU, against a Python reading of PloidyInfo.GetReferenceCopyNumber."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("canvas_partition_states_cbs", "canvas_partition_states_breakpoints", "canvas_reference_copy_numbers", "canvas_call_somatic_ids")
INVALID = -1
P = lambda a: a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def lib():
    from canvas_amd import build
    so, _ = build.build()
    return ctypes.CDLL(so)


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "canvas_hip.h")).read(), flags=re.S)


def test_symbols_declared_listed_exported_and_in_the_csharp_binding(lib):
    from canvas_amd import build
    from canvas_amd.lib import ABI_SYMBOLS
    declared = set(re.findall(r"\b(canvas_\w+)\s*\(", _header()))
    cs = open(os.path.join(ROOT, "hosts", "CanvasHip.cs")).read()
    for name in NEW:
        assert name in declared and name in ABI_SYMBOLS and hasattr(lib, name), name
        assert re.search(r"extern int %s\(" % name, cs), name
        n_header = len(re.search(r"int32_t %s\((.*?)\);" % name, _header(), flags=re.S).group(1).split(","))
        n_cs = len(re.search(r"extern int %s\((.*?)\);" % name, cs, flags=re.S).group(1).split(","))
        assert n_header == n_cs == {"canvas_partition_states_cbs": 6, "canvas_partition_states_breakpoints": 6, "canvas_reference_copy_numbers": 9, "canvas_call_somatic_ids": 32}[name], name
    src = [s for s in build.PRODUCT_SRC if 'extern "C" int32_t canvas_partition_states_cbs(' in open(os.path.join(build.CSRC, s)).read()]
    assert len(src) == 1
    text = open(os.path.join(build.CSRC, src[0])).read()
    assert "__global__" in text and 'extern "C" int32_t canvas_partition_states_breakpoints(' in text


def test_python_surface():
    from canvas_amd import Canvas, lib as L
    assert callable(Canvas.partition_states) and callable(Canvas.call_somatic_ids) and callable(Canvas.somatic_flow) and callable(L.reference_copy_numbers)
    sig = inspect.signature(Canvas.germline_flow).parameters
    assert sig["method"].default == "hmm" and sig["partition"].default is None
    assert list(inspect.signature(Canvas.partition_states).parameters)[1:] == ["chr_offset", "seg_len", "nseg", "breakpoints", "out"]
    flow = list(inspect.signature(Canvas.somatic_flow).parameters)
    tn = list(inspect.signature(Canvas.tumor_normal_flow).parameters)
    assert flow[:9] == tn[:9] and flow[9:14] == ["chr_site_offset", "site_pos", "site_ref", "site_alt", "genome_length"] and {"excluded", "ploidy"} <= set(flow)


def _breakpoints(lib, off, bp, bo, ctx=None):
    off = np.array(off, np.int64); bp = np.array(bp + [0], np.int32); bo = np.array(bo, np.int64)
    lib.canvas_partition_states_breakpoints.argtypes = [ctypes.c_void_p, ctypes.c_int32] + [ctypes.c_void_p] * 4
    return lib.canvas_partition_states_breakpoints(ctx, len(off) - 1, P(off), P(bp), P(bo), ctypes.c_void_p(64))      # 64 stands for a device pointer: never followed on the host


def test_breakpoints_entry_refuses_bad_arguments_before_it_looks_at_the_context(lib):
    """every refusal below is decided on the host arguments alone: the context is NULL and the state pointer is not one, so a call that launched anything, or followed
    either, would not come back with CANVAS_ERR_INVALID"""
    good = dict(off=[0, 12, 12, 30], bp=[3, 11, 0, 17], bo=[0, 2, 2, 4])
    assert _breakpoints(lib, **good) == INVALID                                  # good tables: refused for the missing context only
    for change in (dict(off=[1, 12, 12, 30]), dict(off=[0, 12, 11, 30]), dict(bo=[1, 2, 2, 4]), dict(bo=[0, 3, 2, 4]),
                   dict(bp=[3, 12, 0, 17]),                                      # a breakpoint at T_c
                   dict(bp=[3, 11, 0, 18]), dict(bp=[-1, 11, 0, 17]),            # ... at T_c of the last chromosome; a negative one
                   dict(bp=[3, 11, 0], bo=[0, 2, 3, 3])):                        # a breakpoint on a chromosome without bins
        assert _breakpoints(lib, **dict(good, **change)) == INVALID, change
    lib.canvas_partition_states_breakpoints.argtypes = None
    assert lib.canvas_partition_states_breakpoints(None, 0, None, None, None, None) == INVALID
    assert lib.canvas_partition_states_cbs(None, 1, None, None, None, None) == INVALID
    assert lib.canvas_call_somatic_ids(*([None] * 32)) == INVALID


def _reference_copy_number(begin, end, records):
    """PloidyInfo.GetReferenceCopyNumber (PloidyInfo.cs:56-72) over getPloidyCounts (:92-110); records None: the chromosome is not in PloidyByChromosome"""
    if records is None:
        return 2
    one_based_start, one_based_end = begin + 1, end
    base_counts = [0] * 5
    base_counts[2] = one_based_end - one_based_start + 1
    for start, stop, ploidy in records:
        if ploidy == 2:
            continue
        overlap_start = max(one_based_start - 1, start - 1)
        if overlap_start > stop:
            continue
        overlap_bases = min(one_based_end, stop) - overlap_start
        if overlap_bases <= 0:
            continue
        base_counts[2] -= overlap_bases
        base_counts[ploidy] += overlap_bases
    best, ref = 0, 2
    for cn in range(5):
        if base_counts[cn] > best:
            best, ref = base_counts[cn], cn
    return ref


def test_reference_copy_numbers_against_ploidy_info():
    from canvas_amd.lib import reference_copy_numbers, CanvasError
    # chromosome 0: no records.  1: a haploid stretch over [1001, 2000] and a record at ploidy 2 that is skipped.  2: copy numbers 0, 3 and 1 side by side.  3: no segment
    ploidy = [((), (), ()), ((1001, 1, 5000), (2000, 400, 9000), (1, 3, 2)), ((1, 501, 1001, 1601), (500, 1000, 1600, 1900), (0, 3, 1, 4)), ((1,), (10,), (1,))]
    segs = [[(0, 100), (100, 100)],
            [(1000, 2000),                         # covered exactly: 1
             (999, 2000), (1000, 2001),            # one base more on either side: still 1 (1 000 of 1 001)
             (1000, 3000),                         # half: 1 000 haploid, 1 000 diploid -> the first of the two, copy number 1
             (1000, 3001),                         # one base fewer than half: 2
             (1000, 2999),                         # one base more than half: 1
             (1500, 1500),                         # End == Begin: every count 0 -> 2
             (0, 300), (0, 700),                   # inside a copy number 3 of 400 bases, and 300 bases past it: 3 both times (400 of 700 > 300)
             (6000, 8000)],                        # under the ploidy-2 record only
            [(0, 500), (0, 1000),                  # copy number 0; a tie of 0 and 3: the first wins
             (400, 700), (250, 1000),              # 100 / 200: 3; 250 / 500: 3
             (500, 1500), (1000, 1900)],           # a tie of 3 and 1 (500 each): the first in copy-number order is 1; 600 of 1 and 300 of 4
            []]
    cso = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.int64)
    beg = np.array([b for s in segs for b, e in s], np.int32); end = np.array([e for s in segs for b, e in s], np.int32)
    got = reference_copy_numbers(cso, beg, end, ploidy)
    want = [_reference_copy_number(b, e, list(zip(*ploidy[c])) if len(ploidy[c][0]) else None) for c, s in enumerate(segs) for b, e in s]
    assert got.dtype == np.int32 and got.tolist() == want
    assert want == [2, 2, 1, 1, 1, 1, 2, 1, 2, 3, 3, 2, 0, 0, 3, 3, 1, 1]
    assert reference_copy_numbers(cso, beg, end, None).tolist() == [2] * len(beg)
    # a chromosome with records behaves like one that is not in the file when none of them overlaps: both give 2
    assert _reference_copy_number(6000, 8000, []) == _reference_copy_number(6000, 8000, None) == 2
    bad = [((), (), ()), ((1,), (10 ** 9,), (5,)), ((), (), ()), ((), (), ())]
    with pytest.raises(CanvasError):
        reference_copy_numbers(cso, beg, end, bad)
    with pytest.raises(CanvasError):
        reference_copy_numbers(cso, beg, end, [((), (), ()), ((1,), (10,), (-1,)), ((), (), ()), ((), (), ())])
