"""CPU restatements of CanvasSmooth (CanvasSmooth/CanvasSmooth.cs:46-77 over CanvasCommon/Utilities.cs:767-791), two of them, written independently of each other:

  smooth_literal   the queue plus the sorted window of Utilities.MedianFilter, value by value, repeated for h = 1 .. W and zipped with the bins
  smooth_windows   the list of index windows the filter's two loops amount to, with numpy sorts and np.float32 arithmetic for the mean of an even window

Both return the smoothed counts of ONE chromosome as a float32 array that is as long as what Enumerable.Zip leaves: shorter than the input when a pass sees fewer
than 2h + 1 values.  out_len is the length recurrence on its own."""
import bisect
from collections import deque

import numpy as np

F32 = np.float32


def next_len(n, h):
    """the number of medians one pass with half window h emits for n values"""
    return n if n >= 2 * h + 1 else max(0, n - h) + max(0, n - h - 1)


def out_len(n, W):
    for h in range(1, W + 1):
        n = next_len(n, h)
    return n


def _sorted_median(window):
    """SortedList<float>.Median(): the middle element, or (a + b) / 2 of the two middle elements, a float"""
    m = len(window)
    if m % 2:
        return F32(window[m // 2])
    return F32((F32(window[m // 2 - 1]) + F32(window[m // 2])) / F32(2))


def median_filter_literal(values, h):
    """Utilities.MedianFilter, statement by statement (the values are kept as Python floats: every float32 is one, and they order the same way)"""
    boundary, size = h + 1, 2 * h + 1
    window, previous, out = [], deque(), []
    for v in values:
        v = float(v)
        if len(window) >= size and previous:
            del window[bisect.bisect_left(window, previous.popleft())]
        bisect.insort(window, v)
        if len(window) >= boundary:
            out.append(_sorted_median(window))
        previous.append(v)
    while len(window) > boundary and previous:
        del window[bisect.bisect_left(window, previous.popleft())]
        out.append(_sorted_median(window))
    return out


def smooth_literal(counts, W):
    bins = list(range(len(counts)))                      # what Enumerable.Zip pairs the counts with
    counts = [F32(c) for c in counts]
    smoothed = counts
    for h in range(1, W + 1):
        smoothed = median_filter_literal(counts, h)
        counts = smoothed
    return np.array([c for _, c in zip(bins, smoothed)], F32)


def _window_median(w):
    """w: a list of floats that are float32 values"""
    s = sorted(w)
    m = len(s)
    return F32(s[m // 2]) if m % 2 else (F32(s[m // 2 - 1]) + F32(s[m // 2])) / F32(2)           # float32 + float32, / float32


def pass_windows(n, h):
    """[(lo, hi)] inclusive, in output order: i = h .. n-1: [max(0, i - 2h), i]; then lo = max(0, n - 1 - 2h) and, while n - lo > h + 1, lo += 1: [lo, n - 1]"""
    out = [(max(0, i - 2 * h), i) for i in range(h, n)]
    lo = max(0, n - 1 - 2 * h)
    while n - lo > h + 1:
        lo += 1
        out.append((lo, n - 1))
    return out


def median_filter_windows(x, h):
    x = np.asarray(x, F32)
    n = len(x)
    if n >= 4 * h + 2:                                   # long: the full windows in one sort, the 2h clamped ones at the ends one by one
        mid = np.sort(np.lib.stride_tricks.sliding_window_view(x, 2 * h + 1), axis=1)[:, h]
        xl = x.tolist()
        head = [_window_median(xl[max(0, j - h):j + h + 1]) for j in range(h)]
        tail = [_window_median(xl[j - h:min(n, j + h + 1)]) for j in range(n - h, n)]
        return np.concatenate([np.array(head, F32), mid.astype(F32), np.array(tail, F32)])
    xl = x.tolist()
    return np.array([_window_median(xl[lo:hi + 1]) for lo, hi in pass_windows(n, h)], F32)


def smooth_windows(counts, W):
    x = np.asarray(counts, F32)
    n0 = len(x)
    for h in range(1, W + 1):
        x = median_filter_windows(x, h)
        if len(x) == 0:
            break
    return x[:n0]


def smooth_genome(counts, offsets, W, one=smooth_windows):
    """every chromosome of a concatenated genome: [smoothed counts of chromosome c]"""
    return [one(counts[int(offsets[c]):int(offsets[c + 1])], W) for c in range(len(offsets) - 1)]
