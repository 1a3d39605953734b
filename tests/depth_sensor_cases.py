"""The case table of the depth sensor tests: input frames built with numpy, parameter sets, buffer layouts.

A case is (shape, parameter set).  `frame_of(shape)` mixes returns, -inf, NaN, +inf, +-0, a positive value, values below min_range
and above max_range, depth steps just under and just over the edge threshold, a lone return inside a miss region, steps across
the kernel's 16 x 64 tile borders, and the values at which the disparity quantisation meets a tie (t = 2, 6) and a zero divisor
(t = 6, 8).  `needs(shape, name)` lists what the oracle must find in the case for it to count (tests/test_depth_sensor_cpu.py).
"""
import numpy as np

MIN_RANGE, MAX_RANGE = 0.5, 10.0
EDGE_ABS, EDGE_REL = 0.05, 0.02
QUANT = 3.0  # 3 / 2 = 1.5 and 3 / 6 = 0.5: ties of rintf; 3 / 6 and 3 / 8 round to 0: the divisor is zero
FRAMES = (0, 1, 0x7FFFFFFF, -1)

# (n, h, w).  The kernel's tile is 16 rows x 64 columns: (1, 17, 65) is one pixel past it both ways
SHAPES = [(1, 1, 1), (2, 1, 5), (2, 5, 1), (3, 3, 3), (2, 7, 37), (2, 9, 64), (1, 17, 65), (3, 30, 40), (1025, 2, 4)]
FULL = [s for s in SHAPES if s[1] >= 7 and s[2] >= 37]  # the shapes that hold the whole pattern


def _p(**kw):
    p = dict(seed=0x123456789ABCDEF, min_range=MIN_RANGE, max_range=MAX_RANGE, edge_radius=0, edge_abs=EDGE_ABS, edge_rel=EDGE_REL,
             edge_drop=0, drop=0, sigma0=0.0, sigma1=0.0, sigma2=0.0, quant=0.0)
    p.update(kw)
    return p


_ALL = dict(edge_radius=2, edge_drop=0x80000000, drop=0x40000000, sigma0=0.01, sigma1=0.005, sigma2=0.002, quant=40.0)
PARAMS = {
    "range_only": _p(),
    "edge_r1_always": _p(edge_radius=1, edge_drop=0xFFFFFFFF),
    "edge_r2_half": _p(edge_radius=2, edge_drop=0x80000000),
    "edge_r1_one": _p(edge_radius=1, edge_drop=1),
    "edge_r2_never": _p(edge_radius=2, edge_drop=0),
    "drop_half": _p(drop=0x80000000),
    "drop_always": _p(drop=0xFFFFFFFF),
    "drop_one": _p(drop=1),
    "noise_s0": _p(sigma0=0.05),
    "noise_s1": _p(sigma1=0.02),
    "noise_s2": _p(sigma2=0.004),
    "quant_tie_zero": _p(quant=QUANT),
    "all": _p(**_ALL),
    "all_other_seed": _p(**dict(_ALL, seed=7)),
}
# [(shape, name)] in a fixed order
CASES = [(s, k) for s in SHAPES for k in PARAMS]


def case_id(case):
    (n, h, w), name = case
    return f"{n}x{h}x{w}-{name}"


def frames_of(case):
    """frame[e]: the four values of the issue in turn, starting at another one for every parameter set"""
    (n, _, _), name = case
    k = list(PARAMS).index(name)
    return np.array([FRAMES[(e + k) % 4] for e in range(n)], np.int32)


def uses_lut(name):
    p = PARAMS[name]
    return p["sigma0"] > 0 or p["sigma1"] > 0 or p["sigma2"] > 0


SPECIALS = [-np.inf, np.nan, -MAX_RANGE * 1.5, -MIN_RANGE / 2, np.inf, 0.0, 2.0, -0.0]  # raw values: MISS, VOID, FAR, VOID ...
SMALL_T = (2.0, 6.0, 8.0, 3.25, 4.5)


def _step(tp, over):
    """t_q > t_p whose step is just under (equal to or one ulp below) or just over the threshold of p"""
    tp = np.float32(tp)
    thr = np.float32(EDGE_ABS) + np.float32(EDGE_REL) * tp
    tq = np.float32(tp + thr)
    if over:
        while not np.abs(np.float32(tq - tp)) > thr:
            tq = np.nextafter(tq, np.float32(np.inf))
    else:
        while np.abs(np.float32(tq - tp)) > thr:
            tq = np.nextafter(tq, np.float32(-np.inf))
    return tq


_FRAMES = {}


def frame_of(shape):
    """-> dict(depth f32 [n,h,w], seg f32 [n,h,w], edge = [(e, v, u)] RET pixels that must be edge pixels at radius 1 and 2,
    calm = [(e, v, u)] RET pixels that must not be).  Built once per shape; do not modify."""
    if shape in _FRAMES:
        return _FRAMES[shape]
    n, h, w = shape
    rng = np.random.default_rng(n * 10007 + h * 101 + w)
    edge, calm = [], []
    if shape in FULL:
        vv, uu = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        t = (3.0 + 0.01 * (uu + vv))[None] + 0.1 * np.arange(n)[:, None, None]
        t = t.astype(np.float32)
        for i, s in enumerate(SPECIALS):
            t[:, 1, 2 + 4 * i] = -np.float32(s)
        t[:, 1, 32], t[:, 1, 34], t[:, 1, 36] = 2.0, 6.0, 8.0
        t[:, 4, 4] = [_step(t[e, 4, 3], False) for e in range(n)]     # (4, 3) sees a step just under its threshold
        t[:, 4, 13] = [_step(t[e, 4, 12], True) for e in range(n)]     # (4, 12) one just over
        calm += [(e, 4, 3) for e in range(n)]
        edge += [(e, 4, 12) for e in range(n)]
        t[:, 4:7, 20:23] = np.inf                                      # a miss region (raw -inf) with a lone return inside
        t[:, 5, 21] = 4.0
        edge += [(e, 5, 21) for e in range(n)]
        calm += [(e, 6, 8) for e in range(n)]
        if w >= 65 and h >= 9:                                          # over the tile's right border: (8, 63) | (8, 64)
            t[:, 8, 64] = [_step(t[e, 8, 63], True) for e in range(n)]
            edge += [(e, 8, 63) for e in range(n)]
        if h >= 17:                                                     # over its lower border: (15, 33) / (16, 33)
            t[:, 16, 33] = [_step(t[e, 15, 33], True) for e in range(n)]
            edge += [(e, 15, 33) for e in range(n)]
            calm += [(e, 15, 10) for e in range(n)]
        if h > 20:                                                      # scattered misses and far returns below the pattern
            m = rng.random((n, h - 20, w))
            t[:, 20:][m < 0.04] = np.inf
            t[:, 20:][m > 0.97] = 12.0
        depth = -t
    else:
        hw = h * w
        depth = np.empty((n, hw), np.float32)
        k = min(len(SPECIALS) - 1, hw - 1)
        for e in range(n):
            for i in range(hw):
                depth[e, (i + e) % hw] = SPECIALS[i - (hw - k)] if i >= hw - k else -SMALL_T[(e + i) % len(SMALL_T)]
        depth = depth.reshape(n, h, w)
    seg = np.where(rng.random((n, h, w)) < 0.7, 255.0, 0.0).astype(np.float32)
    seg.reshape(-1)[::7] = 3.5  # seg is copied as bits, whatever it holds
    _FRAMES[shape] = dict(depth=np.ascontiguousarray(depth, np.float32), seg=seg, edge=edge, calm=calm)
    return _FRAMES[shape]


def needs(shape, name):
    """The masks of the oracle's info (plus "noisy", "quantised", "calm_ret") that must be non-empty for the case to count."""
    n, h, w = shape
    p = PARAMS[name]
    hw = h * w
    out = ["ret"] + (["miss", "void", "far"] if hw >= 5 else [])
    many = n * hw >= 1000  # enough RET pixels that a threshold of one half certainly lands on both sides
    if p["edge_radius"] > 0 and hw >= 5:
        out.append("edge")
        if shape in FULL:
            out.append("calm_ret")
        if p["edge_drop"] == 0xFFFFFFFF or (p["edge_drop"] >= 0x40000000 and many):
            out.append("edge_dropped")
        if p["edge_drop"] != 0xFFFFFFFF and many:
            out.append("edge_kept")
    if p["drop"] == 0xFFFFFFFF or (p["drop"] >= 0x40000000 and many):
        out.append("rand_dropped")
    if p["drop"] in (0, 1) and (p["edge_radius"] == 0 or p["edge_drop"] in (0, 1)) or \
            (many and p["drop"] != 0xFFFFFFFF and (shape in FULL or p["edge_radius"] == 0 or p["edge_drop"] != 0xFFFFFFFF)):
        out.append("kept")  # (a threshold of 1 drops a pixel once in 2^32)
    if uses_lut(name):
        out.append("noisy")
    if p["quant"] > 0:
        out.append("quantised")
        if name == "quant_tie_zero" and hw >= 5:
            out += ["tie", "zero_divisor", "beyond"]
    return out


# buffer layouts of the GPU test: (env stride of the input, of the output, floats in front of the first block); both above h w.
# "wide": strides and offsets that keep 16-byte alignment (the 16-byte path wherever w % 4 == 0); "odd": nothing aligned
def layout(shape, kind):
    hw = shape[1] * shape[2]
    if kind == "wide":
        r = (hw + 3) // 4 * 4
        return r + 4, r + 8, 16
    return hw + 3, hw + 5, 5


LAYOUTS = ("wide", "odd")


# ---- shared by tests/test_depth_sensor_cpu.py and tests/test_depth_sensor_gpu.py
_ORACLE = {}


def oracle(case):
    """The oracle's result of a case, computed once and shared by the CPU and the GPU tests; do not modify."""
    if case not in _ORACLE:
        shape, name = case
        from tests import depth_sensor_oracle as DO
        f = frame_of(shape)
        lut = DO.gauss_table().astype(np.float32) if uses_lut(name) else None
        _ORACLE[case] = DO.sensor(f["depth"], f["seg"], frames_of(case), PARAMS[name], lut=lut)
    return _ORACLE[case]


IN_D, IN_S, OUT_D, OUT_S = 0x100000, 0x200000, 0x300000, 0x400000  # made-up addresses, 1 MiB apart; a frame spans 2 * 5000 * 4 bytes


def base_args(**kw):
    """A GnbvDepthSensor that the library accepts (tests/test_depth_sensor_gpu.py runs the same values on real buffers), on made-up
    pointers: the CPU test changes one field at a time, and every such call is refused before a launch could follow."""
    from gennbv_amd import _lib
    a = _lib.GnbvDepthSensor()
    a.n, a.h, a.w = 2, 60, 80
    a.depth_in, a.seg_in, a.depth_out, a.seg_out = IN_D, IN_S, OUT_D, OUT_S
    a.in_env_stride, a.out_env_stride = 5000, 5000
    a.frame, a.gauss_lut, a.seed = 0x500000, 0x600000, 5
    a.min_range, a.max_range, a.edge_radius, a.edge_abs, a.edge_rel = 0.5, 10.0, 1, 0.05, 0.02
    a.edge_drop, a.drop, a.sigma0, a.sigma1, a.sigma2, a.quant = 0x80000000, 1000, 0.01, 0.0, 0.001, 40.0
    for f, v in kw.items():
        setattr(a, f, v)
    return a
