"""Helpers of the GPU tests that call the C ABI directly and bound the error element by element (tests/test_linear_gpu.py,
tests/test_dense_path_gpu.py): NaN-prefilled outputs with a sentinel tail, and the largest err / bound ratio of a result."""
import math

import torch

from gennbv_amd import _lib

DEV = "cuda:0"
TAIL, SENTINEL = 64, 1234.5


def _stream():
    return _lib.stream_ptr(torch.device(DEV))


def _out(*shape, dtype=torch.float32):
    """An output buffer prefilled with NaN and followed by a TAIL-element sentinel: (the output view, the whole buffer)."""
    n = math.prod(shape)
    buf = torch.full((n + TAIL,), float("nan"), dtype=dtype, device=DEV)
    buf[n:] = SENTINEL
    return buf[:n].view(*shape), buf


def _check_written(name, body, buf):
    n = body.numel()
    bad = int((~torch.isfinite(body)).sum())
    assert bad == 0, f"{name}: {bad} of {n} elements not written or not finite"
    assert bool((buf[n:] == SENTINEL).all()), f"{name}: the {TAIL} elements past the output were written"


def _ratio(got, want, bound):
    """Largest |got - want| / bound (an element whose bound is 0 must be exact)."""
    err = (got.double() - want).abs()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0))
    return float(r.max())


def _report(what, ratios):
    line = f"[err/bound] {what}: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items())
    print(line)
    return line
