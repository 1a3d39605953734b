"""CPU checks of k_conv2_dgrad_c1w_split's class epilogue (csrc/conv_split.h, no GPU).

* relu_threshold: the BN1 ReLU mask fmaf(sc, y, sh) > 0 replaced by ONE compare, (y > thr) != (sc < 0).  A Python model of the kernel's
  bisection, with an exact oracle for the fma sign, checked over every sign of sc / sh, +-0, subnormal and huge values.
* ISA: the kernel keeps 0 bytes of scratch, <= 128 VGPRs and 4 waves per SIMD (any spill has cost these kernels several times over).
"""
import math
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)

F32_MAX = float(np.finfo(np.float32).max)
TINY = Fraction(1, 2 ** 150)  # half the smallest f32 subnormal


def f32(x) -> float:
    return float(np.float32(x))


def fma_pass(sc: float, y: float, sh: float) -> bool:
    """fmaf(sc, y, sh) > 0 for finite f32 operands: the exact sum rounded once to f32 is positive iff it exceeds 2^-150 (exactly
    2^-150 is a tie that rounds to the even 0).  (In float64 sc * y is exact but the sum is rounded once more: the exact value is
    needed in the underflow window.)"""
    if math.isnan(sc) or math.isnan(sh):
        return False
    return Fraction(sc) * Fraction(y) + Fraction(sh) > TINY


def from_key(k: int) -> float:
    bits = (k & 0x7FFFFFFF) if (k & 0x80000000) else (~k & 0xFFFFFFFF)
    return float(np.array([bits], dtype=np.uint32).view(np.float32)[0])


def to_key(f: float) -> int:
    bits = int(np.array([f], dtype=np.float32).view(np.uint32)[0])
    return (bits | 0x80000000) if not (bits & 0x80000000) else (~bits & 0xFFFFFFFF)


def relu_threshold(sc: float, sh: float):
    """Model of relu_threshold in csrc/conv_split.h: 32 bisection steps over the order keys of the finite floats."""
    flip = sc < 0.0
    k_lo, k_hi = 0x00800000, 0xFF7FFFFF
    lo, hi = k_lo, k_hi + 1
    for _ in range(32):
        mid = lo + ((hi - lo) >> 1)
        if lo < hi:  # (the kernel evaluates the predicate here too -- at mid = +inf once converged -- and discards it)
            t = fma_pass(sc, from_key(mid), sh) != flip
            hi, lo = (mid, lo) if t else (hi, mid + 1)
    assert lo == hi
    return (-math.inf if lo == k_lo else from_key(lo - 1)), flip


def one_compare(y: float, thr: float, flip: bool) -> bool:
    return (y > thr) != flip


SUB_MIN, SUB_MAX, NORM_MIN = 2.0 ** -149, f32(2.0 ** -126 - 2.0 ** -149), 2.0 ** -126
MAGS = [f32(v) for v in (0.0, SUB_MIN, 3 * SUB_MIN, SUB_MAX, NORM_MIN, 2.0 ** -100, 1e-20, 0.37, 1.0, 1.5, 3.0, 1e10, 2.0 ** 100, F32_MAX)]
SIGNED = sorted({s * m for m in MAGS for s in (1.0, -1.0)} | {-0.0}, key=lambda v: (v, math.copysign(1.0, v)))


def y_probe(thr: float):
    """Finite floats around the threshold (its neighbours on both sides) and across the whole range."""
    ys = list(SIGNED)
    if math.isfinite(thr):
        k = to_key(thr)
        for d in range(-3, 4):
            if 0x00800000 <= k + d <= 0xFF7FFFFF:
                ys.append(from_key(k + d))
    return ys


def test_key_order_is_the_float_order():
    vals = sorted(SIGNED + [from_key(k) for k in (0x00800000, 0xFF7FFFFF)], key=lambda v: (v, math.copysign(1.0, v)))  # -0 before +0
    keys = [to_key(v) for v in vals]
    assert keys == sorted(keys)
    assert from_key(0x00800000) == -F32_MAX and from_key(0xFF7FFFFF) == F32_MAX
    assert all(from_key(to_key(v)) == v for v in SIGNED)


@pytest.mark.parametrize("sc", SIGNED)
def test_threshold_equals_fma_sign_for_edge_scales_and_shifts(sc):
    for sh in SIGNED:
        thr, flip = relu_threshold(sc, sh)
        assert flip == (sc < 0.0)
        for y in y_probe(thr):
            assert one_compare(y, thr, flip) == fma_pass(sc, y, sh), (sc, sh, y, thr, flip)


def test_threshold_equals_fma_sign_for_random_bn_parameters():
    rng = np.random.default_rng(7)
    for _ in range(150):
        sc = f32(rng.standard_normal() * 10.0 ** rng.integers(-3, 3))
        sh = f32(rng.standard_normal() * 10.0 ** rng.integers(-3, 3))
        thr, flip = relu_threshold(sc, sh)
        ys = y_probe(thr) + [f32(v) for v in rng.standard_normal(20) * 4.0]
        for y in ys:
            assert one_compare(y, thr, flip) == fma_pass(sc, y, sh), (sc, sh, y, thr, flip)


def test_threshold_never_passes_for_nan_parameters():
    for sc, sh in ((math.nan, 1.0), (1.0, math.nan), (-1.0, math.nan)):
        thr, flip = relu_threshold(sc, sh)
        assert not any(one_compare(y, thr, flip) for y in SIGNED)


@pytest.mark.skipif(HIPCC is None, reason="hipcc needed to compile the gfx950 kernels")
def test_dgrad_split_kernel_has_no_scratch_and_full_occupancy():
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fvisibility=hidden",
           "-I" + os.path.join(ROOT, "include"), "--cuda-device-only", "-c", os.path.join(ROOT, "gennbv_amd", "csrc", "encoder.hip"),
           "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    # remarks per kernel: "Function Name: <mangled>", then "VGPRs: n", "ScratchSize [bytes/lane]: n", "Occupancy [waves/SIMD]: n"
    blocks = re.split(r"remark: Function Name: ", r.stderr)[1:]
    found = {}
    for b in blocks:
        name = b.split()[0]
        if name.startswith("_Z23k_conv2_dgrad_c1w_split"):
            get = lambda key: int(re.search(re.escape(key) + r"\s*(\d+)", b).group(1))
            found[name] = (get("VGPRs:"), get("ScratchSize [bytes/lane]:"), get("Occupancy [waves/SIMD]:"))
    assert len(found) == 1, list(found)
    vgpr, scratch, occ = next(iter(found.values()))
    assert scratch == 0 and vgpr <= 128 and occ == 4, (vgpr, scratch, occ)
