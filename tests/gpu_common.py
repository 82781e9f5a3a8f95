"""helpers shared by the -m gpu tests"""
import numpy as np
import pytest


def get_canvas():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from canvas_amd import Canvas
    return Canvas(0)


def to_dev(a, device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def pad16(a):
    n = (len(a) + 63) // 64 * 64
    out = np.zeros(n, a.dtype)
    out[:len(a)] = a
    return out


def wavelets_coverage(rng, n, mean=100.0, events=6, wave=0.0):
    """a chromosome's coverage for the Wavelets tests: Poisson counts with a few scaled or zeroed stretches and an optional slow wave, as two-decimal values"""
    x = rng.poisson(mean, n).astype(np.float64)
    for _ in range(events if n > 40 else 0):
        a = int(rng.randint(0, n - 20)); b = min(n, a + int(rng.choice([12, 40, 300, 2500, n // 4 + 1])))
        x[a:b] = np.round(x[a:b] * float(rng.choice([0.0, 0.5, 1.5, 2.0])))
    if wave:
        x = np.round(x * (1 + wave * np.sin(np.arange(n) / 700.0)))
    return np.round(x * 100) / 100      # what the cleaned file holds: F2 text
