"""CPU: the launch plan of the encoder grid branch.  csrc/encoder_plan.h is the host code that decides, per call, which conv / BN /
gradient kernel every stage runs, on what grid, and where it keeps its scratch; tests/encoder_plan_dump.cpp, compiled here with the
host compiler under the address and undefined-behaviour sanitizers and run as a process of its own, prints its plans.  The knobs
reach it as environment strings, so the parsing is the library's too.

* cases: for every case of tests/test_encoder_abi_gpu.py the planned paths are the ones the GPU test's mirror (_paths) states;
* thresholds: a sweep over G x input form x mode x autocorrelation x each knob alone x force_fp32 against `want`, a restatement of
  the conditions the front end had before the plan existed, written out below in that code's order;
* grids: workgroup caps, the MAXWG knobs with their out-of-range values, where the x-tiled kernels switch to their loop forms;
* forward / backward agreement, and the workspace layout against its formulas, with the overlaps it documents.

One boundary of the old code has only one side: 2 O1 + 1 <= G holds for every G (O1 = (G - 3) / 2 + 1 gives G - 1 or G), which
test_thresholds asserts instead of looking for a G beyond it."""
import itertools
import json
import os
import shutil
import subprocess
from collections import namedtuple

import pytest

from tests.encoder_abi_cases import CASES, KNOBS, _paths

HERE = os.path.dirname(os.path.abspath(__file__))
STATE_DIM = 600  # (tests/test_encoder_abi_gpu.py: the grid slice of an observation row starts here)
E1, E1F, E2, AC_ROW = 528, 544, 6928, 768
T = namedtuple("T", "b g train inp ac force dp glob prep feats env", defaults=(True, "rows", None, False, False, False, False, True, ()))
KNOB_VALUES = {"GENNBV_CONV_SPLIT": ["0"], "GENNBV_SPLITX": ["0", "1"], "GENNBV_SPLITX_MAXWG": ["8", "256", "512", "7", "513", "13"],
               "GENNBV_WGRAD_DMA": ["0"], "GENNBV_CONV_MAXWG": ["8", "256", "512", "7", "513", "13"], "GENNBV_FUSED_BWD": ["0"],
               "GENNBV_CONV1_SPLIT": ["0"], "GENNBV_FUSED_TRAIN": ["0"], "GENNBV_FUSED_EVAL": ["0"], "GENNBV_ANALYTIC_BN1": ["0"]}
assert set(KNOB_VALUES) == set(KNOBS)
ENVS = [()] + [((k, v),) for k in KNOBS for v in KNOB_VALUES[k]]


def _line(t):
    """The dump program's input for t: fp32 rows at the GPU test's row stride ("unaligned": one float further), int8 rows aligned."""
    stride = STATE_DIM + t.g ** 3 + 8192 + (t.inp == "unaligned")
    obs, i8 = t.inp != "compact", t.inp in ("i8", "compact")
    facts = [t.b, t.g, t.train, obs, 4 if t.inp == "unaligned" else 0, stride % 4 if obs else 0, i8, 0, 0, t.ac is not None, t.ac == "total",
             t.glob, t.force, t.dp, t.prep, t.feats]
    env = dict(t.env)
    return " ".join([str(int(v)) for v in facts] + [env.get(k, "-") for k in KNOBS])


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """tuples -> iterator of (tuple, what the sanitised dump program printed for it), one process per call."""
    gxx, hipcc = shutil.which("g++"), shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    cc = [gxx] if gxx else [hipcc, "-x", "c++"] if os.path.exists(hipcc) else None
    if cc is None:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("encoder_plan")
    exe = str(tmp / "encoder_plan_dump")
    subprocess.run(cc + ["-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         os.path.join(HERE, "encoder_plan_dump.cpp"), "-o", exe], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("GENNBV_")}

    def run(tuples):
        tuples = list(tuples)
        run = subprocess.run([exe], input="".join(_line(t) + "\n" for t in tuples), capture_output=True, text=True, env=env)
        assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stderr[-2000:])  # (a sanitizer report goes to stderr)
        lines = run.stdout.splitlines()
        assert len(lines) == len(tuples)
        return ((t, json.loads(l)) for t, l in zip(tuples, lines))
    return run


# ---------------------------------------------------------------------------
# the front end's conditions as they stood before the plan, in that code's order
# ---------------------------------------------------------------------------
def _spg(b, o):
    return (b + 7) // 8 * 8 * o


def _spgg(b, o, pz):
    return (b + 7) // 8 * 8 * -(-o // pz)


def _slices(p):
    return min(max(p // 32, 1), 64)


def want(t):
    g, b, env = t.g, t.b, dict(t.env)
    off = lambda k: env.get(k, "")[:1] == "0"  # noqa: E731

    def maxwg(k, dflt):
        v = int(env.get(k, "0"))
        return v & ~7 if 8 <= v <= 512 else dflt
    o1 = (g - 3) // 2 + 1
    o2, xh = (o1 - 3) // 2 + 1, (o1 + 1) // 2
    p2 = o2 ** 3
    stride = STATE_DIM + g ** 3 + 8192 + (t.inp == "unaligned")
    obs, i8 = t.inp != "compact", t.inp in ("i8", "compact")
    obs_vec = obs and g % 4 == 0 and stride % 4 == 0 and t.inp != "unaligned"
    i8_rows = i8 and g % 16 == 0
    sx = env.get("GENNBV_SPLITX", "")
    split = not off("GENNBV_CONV_SPLIT") and not t.force and xh == 16 and o2 <= 15
    splitx = (not (off("GENNBV_CONV_SPLIT") or t.force or o2 < 1) and sx[:1] != "0"
              and ((16 < xh <= 32 and o2 <= 32) or (xh == 16 and o2 <= 15 and sx[:1] == "1")))
    fused = not off("GENNBV_FUSED_BWD") and i8_rows and 3 * g * g <= 64 * 1024
    c1_lds = 3 * (2 * o1 + 1) * g * 4
    i8_staged = i8_rows and c1_lds <= 64 * 1024 and 2 * o1 + 1 <= g
    analytic_bn1 = t.ac is not None and i8_staged and 3 * g * g <= 64 * 1024 and not off("GENNBV_ANALYTIC_BN1")
    nitems = _spgg(b, o2, 4)
    # ---- forward ----
    f = dict(refusal="none", nitems=0, c1_lds=0, c1_grid=_spg(b, o1))
    dp = t.train and t.dp
    fused_eval = not t.train and split and i8_staged and g == 64 and not off("GENNBV_FUSED_EVAL")
    analytic = fused_train = False
    if fused_eval:
        f.update(bn1="prepared" if t.prep else "prepare", conv1="fused", nitems=nitems, c1_grid=min(nitems, maxwg("GENNBV_CONV_MAXWG", 256)))
    else:
        analytic = t.train and analytic_bn1
        if dp and not (analytic and fused and t.glob):
            f["refusal"] = "dp"
        fused_train = analytic and split and g == 64 and not off("GENNBV_CONV1_SPLIT") and not off("GENNBV_FUSED_TRAIN")
        c1_part = t.train and not analytic
        f.update(bn1="analytic" if analytic else "reduce" if t.train else "finalize", bn1_grid=9 if fused_train else 1,
                 have_total=int(t.ac == "total" and not dp), c1_part=int(c1_part), split_img=int(split or splitx))
        if fused_train:
            f.update(conv1="fused", nitems=nitems, c1_grid=min(nitems, maxwg("GENNBV_CONV_MAXWG", 256)))
        elif i8_staged and not c1_part and g == 64 and split and not off("GENNBV_CONV1_SPLIT"):
            f.update(conv1="split")
        elif i8_staged:
            f.update(conv1="lds_i8", c1_lds=c1_lds)
        elif obs_vec and c1_lds <= 64 * 1024 and 2 * o1 + 1 <= g:
            f.update(conv1="lds_f32", c1_lds=c1_lds)
        elif i8_rows and c1_lds // 4 <= 64 * 1024 and 2 * o1 + 1 <= g:
            f.update(conv1="lds_i8_slab", c1_lds=c1_lds // 4)
        else:
            f.update(conv1="direct_f32" if obs else "direct_i8")
    pz2 = next((pz for pz in (1, 2) if _spgg(b, o2, pz) <= 512), 4)
    if fused_eval or fused_train:
        f.update(conv2="fused", g2=nitems)
    elif splitx:
        f.update(conv2="splitx", g2=_spgg(b, o2, 4) * -(-o2 // 16), XT=-(-o2 // 16))
    elif split:
        f.update(conv2="split", g2=nitems)
    else:
        f.update(conv2="fp32", g2=_spgg(b, o2, pz2), pz2=pz2)
    f["bn2"] = "dp" if dp else "reduce" if t.train else "none" if fused_eval and t.prep else "finalize"
    f["feat_grid"] = min(-(-b * 16 * p2 // 256), 4096) if t.feats else 0
    paths = dict(split=int(split), splitx=int(splitx), fused_bwd=int(fused), i8_staged=int(i8_staged), analytic=int(analytic),
                 fused_eval=int(fused_eval), fused_train=int(fused_train))
    # ---- backward (of a training forward) ----
    saved_total = fused and analytic_bn1
    w = dict(refusal="dp" if t.dp and not (fused and t.glob and saved_total) else "none", saved_total=int(saved_total),
             autocorr_launch=int(fused and not saved_total and t.ac is None), bn2_apply_grid=b * -(-p2 // 64))
    if splitx:
        xt = -(-o2 // 16)
        n = _spgg(b, o2, 4) * xt
        loop = n > 2048 or maxwg("GENNBV_SPLITX_MAXWG", 512) < 512
        w.update(wgrad2="splitx_loop" if loop else "splitx", wg_blocks=min(n, maxwg("GENNBV_SPLITX_MAXWG", 512)) if loop else n, wg_nitems=n, XT=xt)
    elif split:
        dma = not off("GENNBV_WGRAD_DMA")
        w.update(wgrad2="split_dma" if dma else "split", wg_blocks=min(nitems, maxwg("GENNBV_CONV_MAXWG", 256)) if dma else nitems, wg_nitems=nitems)
    else:
        blocks = -(-b * o2 * o2 // 16)
        w.update(wgrad2="fp32", wg_blocks=512 if blocks > 512 else (blocks + 7) & ~7)
    w["wg_slices"] = _slices(w["wg_blocks"])
    ngd = -(-xh // 4)
    pzd = 4 if fused else -(-xh // ngd)
    w.update(pzd=pzd, gd=_spgg(b, xh, pzd))
    if fused and splitx:
        xt = -(-xh // 16)
        n = _spgg(b, xh, 4) * xt
        loop = n * E1F > 1536 * E2 or maxwg("GENNBV_SPLITX_MAXWG", 512) < 512
        w.update(dgrad="fused_splitx_loop" if loop else "fused_splitx", gd=min(n, maxwg("GENNBV_SPLITX_MAXWG", 512)) if loop else n, dg_nitems=n,
                 dg_XT=xt)
    elif fused:
        w.update(dgrad="fused_split" if split else "fused_fp32")
    else:
        w.update(dgrad="plain")
    if fused:
        w.update(wgrad1="fused", wg1_slices=_slices(w["gd"]))
        return paths, f, w
    blocks1 = -(-b * o1 * o1 // 20)
    c1w_lds = 4 * (2 * xh * 16 + 9 * g) * 4
    nr, ni = (2 * xh * 16 + 255) // 256, (9 * g + 255) // 256
    w.update(wg1_blocks=2048 if blocks1 > 2048 else (blocks1 + 7) & ~7)
    w["wg1_slices"] = _slices(w["wg1_blocks"])
    if i8_rows and 9 * g <= 1024 and c1w_lds <= 64 * 1024 and nr <= 4:
        w.update(wgrad1="lds_i8", NR=1 if nr <= 1 else 2 if nr <= 2 else 4, NI=1, c1w_lds=c1w_lds)
    elif obs_vec and c1w_lds <= 64 * 1024 and nr <= 4 and ni <= 5:
        rn = (1, 1) if nr <= 1 and ni <= 1 else (1, 2) if nr <= 1 and ni <= 2 else (2, 3) if nr <= 2 and ni <= 3 else (4, 5)
        w.update(wgrad1="lds_f32", NR=rn[0], NI=rn[1], c1w_lds=c1w_lds)
    else:
        w.update(wgrad1="direct_f32" if obs else "direct_i8")
    return paths, f, w


def _check(t, d):
    """Every stage of both plans of d is the one `want` states for t (compared by stage, so a failure names stage and tuple)."""
    paths, f, w = want(t)
    for name, exp, got in (("paths", paths, d["paths"]), ("fwd", f, d["fwd"]), ("bwd", w, d["bwd"])):
        for k, v in exp.items():
            assert got[k] == v, f"{name}.{k}: plan {got[k]!r}, expected {v!r} for {t}"
    return paths, f, w


# ---------------------------------------------------------------------------
def test_plan_paths_of_every_gpu_case(dump):
    """What tests/test_encoder_abi_gpu.py assumes each of its cases runs (_paths) is what the library plans for it."""
    cases = [c.values[0] for c in CASES]
    tuples = [T(cs["b"], cs["g"], cs["train"], cs["inp"], cs["ac"], cs["force"], prep=bool(cs["prep"]), feats=cs["feats"],
                env=tuple(sorted(cs["env"].items()))) for cs in cases]
    assert len(tuples) == len(CASES) >= 61
    for cs, (t, d) in zip(cases, dump(tuples)):
        p, m = d["paths"], _paths(cs)
        got = dict(split_fwd=p["split"] or p["splitx"] or p["fused_eval"] or p["fused_train"], split_wg=p["split"] or p["splitx"],
                   split_dg=p["fused_bwd"] and (p["split"] or p["splitx"]), fused_bwd=p["fused_bwd"], analytic=p["analytic"],
                   fused_eval=p["fused_eval"])
        assert {k: bool(v) for k, v in got.items()} == {k: bool(v) for k, v in m.items()}, cs
        assert (d["eval_prepare"] == "none") == bool(m["fused_eval"]) or cs["train"], cs
        _check(t, d)


def test_thresholds(dump):
    """The sweep.  `seen` collects (what, G) so that both sides of every boundary are known to have been crossed."""
    grids = list(range(7, 151)) + [160]
    tuples = [T(3, g, train, inp, ac, force, env=env) for g in grids for inp in ("rows", "i8", "compact", "unaligned") for train in (True, False)
              for ac in (None, "rows", "total") for env in ENVS for force in (False, True)]
    seen = set()
    for t, d in dump(tuples):
        paths, f, w = _check(t, d)
        g, o1 = t.g, (t.g - 3) // 2 + 1
        assert 2 * o1 + 1 <= g
        # forward / backward agreement: what the layer-1 buffer and bn_state hold
        assert all(d["bwd"][k] == d["fwd"][k] for k in ("split", "splitx", "fused_bwd")), t
        assert not t.train or d["bwd"]["saved_total"] == d["fwd"]["saved_total"] == (paths["fused_bwd"] and paths["analytic"]), t
        assert d["fwd"]["refusal"] == d["bwd"]["refusal"] == "none"
        if not t.env and not t.force:
            seen |= {("split", g, paths["split"]), ("splitx", g, paths["splitx"]), ("conv2", g, f["conv2"]), ("fused_bwd", t.inp, g, paths["fused_bwd"])}
        if not t.force:
            seen.add(("conv1", t.inp, g, f["conv1"]))
        if t.env in ((), (("GENNBV_FUSED_BWD", "0"),)) and not t.force:
            seen |= {("wgrad1", t.inp, g, w["wgrad1"], w.get("NR"), w.get("NI"))}
    # XH = 16: G 63..66
    assert all(("split", g, 1) in seen for g in (63, 64, 65, 66)) and ("split", 62, 0) in seen and ("split", 67, 0) in seen
    # XH 17..32: G 67..130, fp32 at 131 and below 63
    assert all(("splitx", g, 1) in seen for g in range(67, 131)) and ("splitx", 66, 0) in seen and ("splitx", 131, 0) in seen
    assert ("conv2", 131, "fp32") in seen and ("conv2", 130, "splitx") in seen and ("conv2", 62, "fp32") in seen
    # 3 G^2 <= 65536
    assert ("fused_bwd", "i8", 144, 1) in seen and ("fused_bwd", "i8", 160, 0) in seen
    # the fp32 slab of conv1: 64 in, 80 out -> the int8 slab (int8 rows) / the generic kernel (fp32 rows)
    assert {("conv1", "i8", 48, "lds_i8"), ("conv1", "i8", 80, "lds_i8_slab"), ("conv1", "rows", 64, "lds_f32"),
            ("conv1", "rows", 80, "direct_f32"), ("conv1", "compact", 66, "direct_i8"), ("conv1", "i8", 64, "fused"),
            ("conv1", "i8", 64, "split"), ("conv1", "unaligned", 64, "direct_f32")} <= seen
    # conv1 weight gradient: requests per lane, and 9 G <= 1024 for its int8 form
    wg1 = [e[1:] for e in seen if e[0] == "wgrad1"]
    nr_i8 = {g: nr for inp, g, v, nr, ni in wg1 if v == "lds_i8"}
    assert (nr_i8[16], nr_i8[32], nr_i8[48], nr_i8[64], nr_i8[80], nr_i8[112]) == (1, 1, 2, 2, 4, 4) and 128 not in nr_i8
    assert ("wgrad1", "i8", 128, "lds_f32", 4, 5) in seen and ("wgrad1", "compact", 128, "direct_i8", None, None) in seen
    rn_f32 = {g: (nr, ni) for inp, g, v, nr, ni in wg1 if v == "lds_f32" and inp == "rows"}
    assert (rn_f32[28], rn_f32[32], rn_f32[36], rn_f32[64], rn_f32[68], rn_f32[84], rn_f32[88], rn_f32[128]) == \
        ((1, 1), (1, 2), (2, 3), (2, 3), (4, 5), (4, 5), (4, 5), (4, 5))
    assert {ni for _, ni in rn_f32.values()} == {1, 2, 3, 5} and {nr for nr, _ in rn_f32.values()} == {1, 2, 4}
    assert ("wgrad1", "rows", 132, "direct_f32", None, None) in seen and ("wgrad1", "rows", 63, "direct_f32", None, None) in seen


def test_grids(dump):
    ac64 = dict(inp="i8", ac="rows")
    mw = ["8", "256", "512", "7", "513", "13"]
    tuples = ([T(128, 64, env=(("GENNBV_CONV_MAXWG", v),), **ac64) for v in mw] + [T(128, 64, train=False, inp="i8", env=(("GENNBV_CONV_MAXWG", v),)) for v in mw]
              + [T(128, 128, env=(("GENNBV_SPLITX_MAXWG", v),), **ac64) for v in mw]
              + [T(b, 128, **ac64) for b in (128, 129, 1216, 1217)]
              + [T(b, 20) for b in (1, 3, 128, 256, 505, 506, 512, 513, 2000)] + [T(b, g) for b in (1, 128) for g in (64, 128)]
              + [T(128, 64, dp=True, glob=True, **ac64), T(128, 64, dp=True, **ac64), T(128, 64, dp=True, glob=True, inp="i8"), T(3, 20, dp=True, glob=True),
                 T(128, 64, train=False, dp=True, inp="i8")])
    out = {t: d for t, d in dump(tuples)}
    for t, d in out.items():
        _check(t, d)
    # min(nitems, MAXWG), out-of-range values -> the defaults
    for v, wg in zip(mw, (8, 256, 512, 256, 256, 8)):
        d = out[T(128, 64, env=(("GENNBV_CONV_MAXWG", v),), **ac64)]
        assert (d["switches"]["conv_maxwg"], d["fwd"]["nitems"], d["fwd"]["c1_grid"], d["fwd"]["g2"], d["bwd"]["wg_blocks"]) == (wg, 512, wg, 512, wg)
        assert out[T(128, 64, train=False, inp="i8", env=(("GENNBV_CONV_MAXWG", v),))]["fwd"]["c1_grid"] == wg
    for v, wg in zip(mw, (8, 256, 512, 512, 512, 8)):
        d = out[T(128, 128, env=(("GENNBV_SPLITX_MAXWG", v),), **ac64)]["bwd"]
        assert (d["wg_nitems"], d["dg_nitems"]) == (2048, 2048)
        assert (d["wgrad2"], d["wg_blocks"], d["dgrad"], d["gd"]) == (("splitx", 2048, "fused_splitx", 2048) if wg == 512 else
                                                                      ("splitx_loop", wg, "fused_splitx_loop", wg))
    # the x-tiled loop forms: more items than wg_part has rows (2 048); more rows of kE1F floats than wg1_part holds
    assert [(out[T(b, 128, **ac64)]["bwd"]["wgrad2"], out[T(b, 128, **ac64)]["bwd"]["wg_blocks"]) for b in (128, 129)] == \
        [("splitx", 2048), ("splitx_loop", 512)]
    assert 19456 * E1F <= 1536 * E2 < 19584 * E1F
    assert [(out[T(b, 128, **ac64)]["bwd"]["dgrad"], out[T(b, 128, **ac64)]["bwd"]["gd"]) for b in (1216, 1217)] == \
        [("fused_splitx", 19456), ("fused_splitx_loop", 512)]
    # caps and rounding up to multiples of 8 at 20^3 (O1 = 9, O2 = 4)
    assert [out[T(b, 20)]["bwd"]["wg_blocks"] for b in (1, 3, 128, 512, 513, 2000)] == [8, 8, 128, 512, 512, 512]
    assert [out[T(b, 20)]["bwd"]["wg1_blocks"] for b in (1, 3, 128, 505, 506, 2000)] == [8, 16, 520, 2048, 2048, 2048]
    assert [out[T(b, 20)]["fwd"]["feat_grid"] for b in (1, 128, 2000)] == [4, 512, 4096] and out[T(128, 64)]["fwd"]["feat_grid"] == 4096
    # planes per workgroup: the fp32 conv2 forward (1, 2, 4 by the grid), the balanced data gradient
    assert [out[T(b, 20)]["fwd"]["pz2"] for b in (1, 128, 256, 512)] == [1, 1, 2, 4]
    assert out[T(128, 20)]["bwd"]["pzd"] == 3 and out[T(128, 20)]["bwd"]["gd"] == 256
    assert all(out[T(b, g)]["bwd"]["pzd"] == 4 for b in (1, 128) for g in (64, 128))
    # the data-parallel refusals
    assert [(out[t]["fwd"]["refusal"], out[t]["bwd"]["refusal"]) for t in tuples[-5:]] == \
        [("none", "none"), ("dp", "dp"), ("dp", "dp"), ("dp", "dp"), ("none", "dp")]
    assert out[tuples[-5]]["fwd"]["bn2"] == "dp" and out[tuples[-5]]["fwd"]["have_total"] == 0


def test_workspace_layout(dump):
    shapes = [(b, g) for b in (1, 3, 9, 128, 512) for g in (7, 20, 64, 128, 131)]
    tuples = [T(b, g, inp=inp, ac=ac, env=env) for b, g in shapes for inp, ac in (("rows", None), ("i8", "rows"), ("i8", None))
              for env in ((), (("GENNBV_FUSED_BWD", "0"),))]
    met = set()
    for t, d in dump(tuples):
        b, g, ws, f, w = t.b, t.g, d["ws"], d["fwd"], d["bwd"]
        o1 = (g - 3) // 2 + 1
        # the formulas gnbv_encoder_workspace_bytes and its carving had
        bn, wg = (b + 8) * o1 * 4 * 2 * 16 * 4, 2048 * E2 * 4
        red = (bn + wg + 255) // 256 * 256
        tmp, w2img = red + 8192 * 8, red + 8192 * 8 + 64 * E2 * 8
        w2split = w2img + 2 * 27 * 256 * 4
        assert ws["total"] == bn + wg + (8192 + 64 * E2) * 8 + 2 * 27 * 256 * 4 + 2 * 14 * 2 * 64 * 16 + 1024 + 8192 + 4096
        exp = dict(bn_part=0, bn_part_bytes=bn, wg_part=bn, wg_part_bytes=wg, wg1_part=bn + 512 * E2 * 4, red=red, S2=red + 128 * 8, S1=red + 192 * 8,
                   Rac=red + 1024 * 8, dy2_absmax=red + 2048 * 8, tmp=tmp, tmp_bytes=64 * E2 * 8, tmp1=tmp + 32 * E2 * 8, w2img=w2img,
                   w2img_dgrad=w2img + 27 * 256 * 4, w2split=w2split, w2split_dgrad=w2split + 1792 * 16, w2split_bounds=w2split + (1792 + 2048) * 16)
        assert {k: ws[k] for k in exp} == exp, t
        assert ws["red"] % 256 == 0
        # the named slots of `red`: pairwise disjoint, inside its 8 192 doubles
        slots = [(ws["S2"], 32 * 8), (ws["S1"], 32 * 8), (ws["Rac"], AC_ROW * 4), (ws["dy2_absmax"], 64 * 128)]
        assert all(ws["red"] <= a and a + n <= ws["red"] + 8192 * 8 for a, n in slots)
        assert all(a + n <= c or c + m <= a for (a, n), (c, m) in itertools.combinations(slots, 2))
        # what the launches of these plans write: rows x row length, by region
        fused = w["wgrad1"] == "fused"
        writes = {"bn_part": max(f["c1_grid"] * 32 * 4 if f["c1_part"] else 0, f["g2"] * 32 * 4, b * 16 * 2 * 4, 0 if fused else w["gd"] * 32 * 4),
                  "wg_part": w["wg_blocks"] * E2 * 4, "wg1_part": w["gd"] * E1F * 4 if fused else w["wg1_blocks"] * E1 * 4,
                  "tmp": w["wg_slices"] * E2 * 8, "tmp1": w["wg1_slices"] * (E1F if fused else E1) * 8, "w2img": 27 * 256 * 4, "w2img_dgrad": 27 * 256 * 4,
                  "w2split": 1792 * 16, "w2split_dgrad": 30720, "w2split_bounds": 1024, "red": 8192 * 8}
        ends = {"bn_part": bn, "wg_part": bn + wg, "wg1_part": bn + wg, "tmp": w2img, "tmp1": w2img}
        spans = {k: (ws[k], ws[k] + n) for k, n in writes.items()}
        assert all(hi <= ends.get(k, ws["total"]) for k, (lo, hi) in spans.items()), (t, spans)
        # regions whose written spans meet are the documented overlaps, each between different launches
        doc = {frozenset((a, c)): (la, lc) for a, la, c, lc in ws["overlaps"]}
        assert set(doc) == {frozenset(("wg_part", "wg1_part")), frozenset(("tmp", "tmp1"))} and all(la != lc for la, lc in doc.values())
        for (a, (alo, ahi)), (c, (clo, chi)) in itertools.combinations(spans.items(), 2):
            if alo < chi and clo < ahi:
                assert frozenset((a, c)) in doc, (t, a, c)
                met.add(frozenset((a, c)))
    assert met == {frozenset(("wg_part", "wg1_part")), frozenset(("tmp", "tmp1"))}  # (both do happen: 128 samples at 128^3)
