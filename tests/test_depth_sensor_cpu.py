"""CPU: the depth sensor's oracle (tests/depth_sensor_oracle.py) against known answers and statistics, the case table of
tests/depth_sensor_cases.py shown non-degenerate by the oracle alone, the struct against the header, the refusals of
gnbv_depth_sensor (all made before any launch, so they need no GPU) and the kernels' resources."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import depth_sensor_cases as DC
from tests import depth_sensor_oracle as DO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
INVALID = 1  # hipErrorInvalidValue


# ------------------------------------------------------------------------------------------------------------------------ Philox
@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, want):
    got = DO.philox4x32_10(counter, key)
    assert " ".join(f"{int(x):08x}" for x in got) == want


def test_philox_is_elementwise():
    c0 = np.arange(5, dtype=np.uint64)
    got = DO.philox4x32_10((c0, 3, np.uint64(0xFFFFFFFF), 0), (11, 12))
    for i in range(5):
        one = DO.philox4x32_10((i, 3, 0xFFFFFFFF, 0), (11, 12))
        assert [int(x[i]) for x in got] == [int(x) for x in one]


# ------------------------------------------------------------------------------------------------------------------------- table
def test_gauss_table():
    from gennbv_amd.ops import depth_sensor as DS
    t64 = DO.gauss_table()
    t = DS.gauss_table().numpy()
    assert t.dtype == np.float32 and t.shape == (4096,) and np.array_equal(t, t64.astype(np.float32))
    assert np.array_equal(t, -t[::-1])                      # antisymmetric
    assert (np.diff(t) > 0).all()                           # strictly increasing
    assert abs(float(t[-1]) - 3.6683292) < 1e-6 and abs(float(t[0]) + 3.6683292) < 1e-6
    assert abs(float(np.std(t.astype(np.float64))) - 0.99984) <= 1e-5
    assert DS.NO_RETURN == float(DO.NO_RETURN) == -2.0 ** -100
    assert [DS.threshold_u32(p) for p in (0.0, 0.5, 1.0)] == [0, 0x80000000, 0xFFFFFFFF]


# -------------------------------------------------------------------------------------------------------------------- statistics
def _stat_frame():
    rng = np.random.default_rng(0)
    return -(1.0 + 8.0 * rng.random((4, 64, 64))).astype(np.float32), np.full((4, 64, 64), 255.0, np.float32)


def test_random_dropout_rate():
    """16 384 RET pixels, drop = 0.25: the count within 6 standard errors (sqrt(16384 * .25 * .75) = 55.4) of 4096."""
    depth, seg = _stat_frame()
    d, s, info = DO.sensor(depth, seg, np.array([0, 1, 2, 3], np.int32), DC._p(seed=2024, drop=0x40000000))
    assert info["ret"].all()
    count = int(info["rand_dropped"].sum())
    print("dropped", count)
    assert abs(count - 4096) <= 333
    assert int((d == DO.NO_RETURN).sum()) == count and int((s == 0).sum()) == count


def test_noise_moments():
    """The z drawn for 16 384 RET pixels: mean within 6 / sqrt(16384) = 0.047 of 0, std within 6 * 0.9998 / sqrt(2 * 16384) = 0.034
    (rounded up) of the table's 0.9998."""
    depth, seg = _stat_frame()
    lut = DO.gauss_table().astype(np.float32)
    d, _, info = DO.sensor(depth, seg, np.array([0, 1, 2, 3], np.int32), DC._p(seed=2024, sigma0=0.01), lut=lut)
    z = info["z"].astype(np.float64)
    print("mean z", z.mean(), "std z", z.std())
    assert abs(z.mean()) <= 0.047
    assert abs(z.std() - 0.9998) <= 0.034
    # and the noise is what left the sensor: t_out - t = fl(0.01 z) to within the rounding of the sum
    t = -depth.astype(np.float64)
    assert np.abs((-d.astype(np.float64) - t) - 0.01 * z).max() < 2e-6


# --------------------------------------------------------------------------------------------------------------------- the rule
def test_classes_and_outputs_of_single_pixels():
    raw = np.array([-3.0, -np.inf, np.nan, np.inf, 0.0, -0.0, 2.0, -0.25, -0.5, -10.0, -10.000001, -3e38, -1e-40], np.float32).reshape(1, 1, -1)
    seg = np.full(raw.shape, 255.0, np.float32)
    P = DC._p()
    d, s, info = DO.sensor(raw, seg, np.zeros(1, np.int32), P)
    NR, NI = float(DO.NO_RETURN), -np.inf
    want = [-3.0, NI, NR, NR, NR, NR, NR, NR, -0.5, -10.0, NI, NI, NR]
    assert d[0, 0].tolist() == want
    assert s[0, 0].tolist() == [255.0 if x in (-3.0, -0.5, -10.0) else 0.0 for x in want]
    assert info["ret"][0, 0].tolist() == [x in (-3.0, -0.5, -10.0) for x in want]
    assert info["miss"].sum() == 1 and info["far"].sum() == 2 and info["void"].sum() == 7


def test_quantisation_tie_and_zero_divisor():
    raw = -np.array([2.0, 6.0, 8.0, 1.0, 3.0], np.float32).reshape(1, 1, -1)
    d, s, _ = DO.sensor(raw, np.ones_like(raw), np.zeros(1, np.int32), DC._p(quant=3.0))
    # 3 / 2 = 1.5 -> 2 (tie to even) -> 1.5;  3 / 6 = 0.5 -> 0 (tie to even) -> +inf -> beyond;  3 / 8 -> 0 -> beyond;  1 -> 1;  3 -> 3
    assert d[0, 0].tolist() == [-1.5, -np.inf, -np.inf, -1.0, -3.0] and s[0, 0].tolist() == [1.0, 0.0, 0.0, 1.0, 1.0]


def test_edge_window_ignores_what_lies_outside_the_image():
    t = np.full((1, 3, 3), 2.0, np.float32)
    ret = np.ones((1, 3, 3), bool)
    for r in (1, 2):
        assert not DO.edge_pixels(t, ret, r, 0.05, 0.02).any()
    ret[0, 0, 0] = False
    assert DO.edge_pixels(t, ret, 1, 0.05, 0.02)[0].tolist() == [[False, True, False], [True, True, False], [False, False, False]]
    e2 = DO.edge_pixels(t, ret, 2, 0.05, 0.02)[0]
    assert e2.reshape(-1)[1:].all() and not e2[0, 0]  # (the pixel itself is not its own neighbour)


# ------------------------------------------------------------------------------------------------------------------- case table
oracle = DC.oracle


def test_the_table_covers_what_the_issue_lists():
    assert set(DC.SHAPES) >= {(1, 1, 1), (2, 1, 5), (2, 5, 1), (3, 3, 3), (2, 7, 37), (2, 9, 64), (1, 17, 65), (3, 30, 40), (1025, 2, 4)}
    ps = DC.PARAMS.values()
    assert {p["edge_drop"] for p in ps} >= {0, 1, 0x80000000, 0xFFFFFFFF} and {p["drop"] for p in ps} >= {0, 1, 0x80000000, 0xFFFFFFFF}
    assert len({p["seed"] for p in ps}) >= 2 and {p["edge_radius"] for p in ps} == {0, 1, 2}
    assert {int(v) for c in DC.CASES for v in DC.frames_of(c)} == {0, 1, 0x7FFFFFFF, -1}
    for shape in DC.SHAPES:
        for kind in DC.LAYOUTS:
            si, so, _ = DC.layout(shape, kind)
            assert si > shape[1] * shape[2] and so > shape[1] * shape[2]
    f = DC.frame_of((3, 30, 40))["depth"]
    for probe in (np.isneginf, np.isnan, np.isposinf, lambda x: (x == 0) & ~np.signbit(x), lambda x: x > 0,
                  lambda x: (-x > 0) & (-x < DC.MIN_RANGE), lambda x: np.isfinite(x) & (-x > DC.MAX_RANGE)):
        assert probe(f).any()


@pytest.mark.parametrize("case", DC.CASES, ids=DC.case_id)
def test_case_is_not_degenerate(case):
    shape, name = case
    P = DC.PARAMS[name]
    d, s, info = oracle(case)
    with np.errstate(all="ignore"):
        q = np.float32(P["quant"]) / info["t1"] if P["quant"] > 0 else np.zeros_like(info["t1"])
        frac = q - np.floor(q)
    ret = info["ret"]
    info = dict(info, edge_kept=info["edge"] & ~info["edge_dropped"], calm_ret=ret & ~info["edge"], noisy=ret & (info["t1"] != info["t"]),
                quantised=ret & (info["t2"] != info["t1"]), tie=ret & (frac == 0.5), zero_divisor=ret & (np.rint(q) == 0) & (P["quant"] > 0))
    for key in DC.needs(shape, name):
        assert info[key].any(), (DC.case_id(case), key)
    f = DC.frame_of(shape)
    if P["edge_radius"] > 0:
        for p in f["edge"]:
            assert info["edge"][p], p
        for p in f["calm"]:
            assert ret[p] and not info["edge"][p], p
    # the outputs follow the masks
    assert np.array_equal(d == DO.NO_RETURN, info["void"] | info["edge_dropped"] | info["rand_dropped"] | info["below"])
    assert np.array_equal(np.isneginf(d), info["miss"] | info["far"] | info["beyond"])
    assert (s[~info["kept"]] == 0).all() and np.array_equal(s.view(np.uint32)[info["kept"]], f["seg"].view(np.uint32)[info["kept"]])


def test_seed_and_frame_change_the_noise():
    a, b = oracle(((3, 30, 40), "all")), oracle(((3, 30, 40), "all_other_seed"))
    assert not np.array_equal(a[0], b[0], equal_nan=True)
    shape = (3, 30, 40)
    f = DC.frame_of(shape)
    lut = DO.gauss_table().astype(np.float32)
    fr = DC.frames_of((shape, "all"))
    again = DO.sensor(f["depth"], f["seg"], fr + 1, DC.PARAMS["all"], lut=lut)
    assert not np.array_equal(a[0], again[0], equal_nan=True)
    # env e of the batch alone, with its own frame counter: the same pixels
    one = DO.sensor(f["depth"][2:3], f["seg"][2:3], fr[2:3], DC.PARAMS["all"], lut=lut, env0=2)
    assert np.array_equal(one[0][0], a[0][2], equal_nan=True) and np.array_equal(one[1][0], a[1][2])


# --------------------------------------------------------------------------------------------------------------- header and ABI
def test_struct_fields_follow_the_header():
    from gennbv_amd import _lib
    from gennbv_amd.csrc import build
    hdr = open(os.path.join(ROOT, "include", "gennbv_hip.h")).read()
    assert re.search(r"\bint\s+gnbv_depth_sensor\s*\(\s*const\s+GnbvDepthSensor\s*\*", hdr)
    assert re.search(r"#define\s+GNBV_DEPTH_NO_RETURN\s+\(-0x1p-100f\)", hdr)
    body = re.search(r"typedef struct GnbvDepthSensor \{(.*?)\} GnbvDepthSensor;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.split(r"[\s\*]+", n.strip())[-1] for decl in body.split(";") if decl.strip() for n in decl.split(",")]
    assert names == [f[0] for f in _lib.GnbvDepthSensor._fields_]
    types = dict(_lib.GnbvDepthSensor._fields_)
    assert types["seed"] is C.c_uint64 and types["edge_drop"] is C.c_uint32 and types["drop"] is C.c_uint32
    assert types["in_env_stride"] is C.c_int64 and types["out_env_stride"] is C.c_int64
    assert _lib.SIGNATURES["gnbv_depth_sensor"] == (C.c_int, [C.c_void_p] * 2)
    lib = _lib.load()
    assert lib.gnbv_depth_sensor is not None and lib.gnbv_abi_version() == 5
    assert "sensor.hip" in build.SOURCES


IN_D, IN_S, OUT_D, OUT_S = DC.IN_D, DC.IN_S, DC.OUT_D, DC.OUT_S
_args = DC.base_args


SPAN = (5000 + 4800) * 4  # bytes of a frame's span
REFUSED = [
    dict(n=0), dict(h=0), dict(w=0), dict(n=-1), dict(in_env_stride=4799), dict(out_env_stride=4799), dict(in_env_stride=0),
    dict(depth_in=None), dict(seg_in=None), dict(depth_out=None), dict(seg_out=None), dict(frame=None), dict(gauss_lut=None),
    dict(min_range=0.0), dict(min_range=-1.0), dict(min_range=11.0), dict(min_range=float("nan")), dict(max_range=float("inf")),
    dict(max_range=float("nan")), dict(edge_radius=-1), dict(edge_radius=3), dict(edge_abs=-0.1), dict(edge_abs=float("inf")),
    dict(edge_rel=-0.1), dict(edge_rel=float("nan")), dict(sigma0=-1.0), dict(sigma1=float("inf")), dict(sigma2=float("nan")),
    dict(quant=-1.0), dict(quant=float("inf")),
    dict(h=65536, w=65536, in_env_stride=2 ** 32, out_env_stride=2 ** 32),  # h w = 2^32
    # overlaps: in place, an output inside an input's span, the two outputs on each other
    dict(depth_out=IN_D), dict(seg_out=IN_S), dict(depth_out=IN_S), dict(seg_out=IN_D), dict(depth_out=IN_D + SPAN - 4),
    dict(depth_out=IN_D - SPAN + 4), dict(seg_out=OUT_D), dict(seg_out=OUT_D + 4800 * 4),
    dict(in_env_stride=10000, out_env_stride=10000, depth_out=IN_D + 5000 * 4),  # interleaved blocks, pairwise disjoint: the test is on the spans
]


def test_refusals_before_any_launch():
    from gennbv_amd import _lib
    lib = _lib.load()
    assert lib.gnbv_depth_sensor(None, None) == INVALID
    for kw in REFUSED:
        assert lib.gnbv_depth_sensor(C.byref(_args(**kw)), None) == INVALID, kw


def test_depth_sensor_refuses_what_it_cannot_run():
    from gennbv_amd import _lib
    from gennbv_amd.ops.depth_sensor import DepthSensor
    with pytest.raises(_lib.GennbvHipError, match="GPU only"):
        DepthSensor(2, 30, 40, min_range_m=0.5, max_range_m=10.0, device="cpu")
    with pytest.raises(_lib.GennbvHipError, match="probability"):
        from gennbv_amd.ops.depth_sensor import threshold_u32
        threshold_u32(1.5)


# --------------------------------------------------------------------------------------------------------------------- resources
@pytest.mark.skipif(HIPCC is None, reason="hipcc needed to compile the gfx950 kernels")
def test_sensor_kernels_compile_for_gfx950_without_scratch():
    from gennbv_amd.csrc import build as B
    cmd = [HIPCC] + B.flags() + ["--cuda-device-only", "-c", os.path.join(ROOT, "gennbv_amd", "csrc", "sensor.hip"), "-o", os.devnull,
                                 "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = {}
    for b in re.split(r"remark: Function Name: ", r.stderr)[1:]:
        get = lambda key: int(re.search(re.escape(key) + r"\s*(\d+)", b).group(1))
        rows[b.split()[0]] = (get("VGPRs:"), get("ScratchSize [bytes/lane]:"), get("LDS Size [bytes/block]:"), get("Occupancy [waves/SIMD]:"))
    assert len(rows) == 6, list(rows)  # edge_radius 0, 1, 2, each with the 16-byte and the dword path
    for name, (vgpr, scratch, lds, occ) in rows.items():
        print(name, "VGPRs", vgpr, "scratch", scratch, "LDS", lds, "waves/SIMD", occ)
        assert "k_depth_sensor" in name and scratch == 0 and occ >= 4, (name, vgpr, scratch, occ)
        assert (lds == 0) == ("ILi0E" in name), (name, lds)  # the no-stencil variants run no LDS code
