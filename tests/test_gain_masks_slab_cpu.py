"""CPU: gnbv_view_gain_slab_masks' export and its refusals (all made before any launch, so they need no GPU), the operator's
refusals, and a numpy model of the word-ownership rule of k_vg_slab<true> / k_vg_prep<true> (csrc/viewgain.hip): which words of a
candidate's row a slab of x-planes stores whole, which it shares with a neighbour and ORs into, and which the prep kernel zeroes."""
import ctypes as C

import numpy as np
import pytest

from gennbv_amd.env import synthetic as S
from gennbv_amd.env.config import TaskConfig
from tests import gain_masks_oracle as MO

INVALID = 1  # hipErrorInvalidValue
SIG = (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p])


def test_library_exports_the_entry_point_and_binds_it():
    from gennbv_amd import _lib
    assert _lib.SIGNATURES["gnbv_view_gain_slab_masks"] == SIG
    lib = _lib.load()
    assert hasattr(lib, "gnbv_view_gain_slab_masks") and lib.gnbv_abi_version() == 5
    assert lib.gnbv_view_gain_slab_masks.argtypes == SIG[1] and lib.gnbv_view_gain_slab_masks.restype is C.c_int


def _args(**kw):
    """A GnbvViewGain the entry point accepts, on made-up non-NULL pointers: every call below is refused before any is read."""
    from gennbv_amd import _lib
    a = _lib.GnbvViewGain()
    a.n, a.k, a.g, a.h, a.w, a.stride, a.range, a.chunk, a.ablate = 2, 3, 72, 60, 80, 4, 50.0, 0, 0
    a.tri_i8 = a.poses = a.range_gt = a.voxel_size = a.inv_intri = a.gain = 0x1000
    a.tri_row_stride = 72 ** 3
    for f, v in kw.items():
        setattr(a, f, v)
    return a


WORDS = MO.min_words(72)  # 11664: 72^3 / 32 exactly
BIG = 1 << 40             # a workspace size no case here exceeds


def test_refusals_before_any_launch():
    from gennbv_amd import _lib
    lib = _lib.load()
    assert WORDS == 11664 and lib.gnbv_view_gain_slab_workspace_bytes(2, 3, 72, 60, 80, 4) > 0

    def call(a, slab=0, ws=0x4000, ws_bytes=BIG, words=WORDS, ub=0x2000, hb=0x3000):
        return lib.gnbv_view_gain_slab_masks(C.byref(a), slab, ws, ws_bytes, words, ub, hb, None)
    assert lib.gnbv_view_gain_slab_masks(None, 0, 0x4000, BIG, WORDS, 0x2000, 0x3000, None) == INVALID
    # everything gnbv_view_gain_slab refuses, with g in 2..128
    for kw in (dict(stride=0), dict(range=0.0), dict(range=float("inf")), dict(k=0), dict(n=0), dict(g=1), dict(g=129, tri_row_stride=129 ** 3),
               dict(gain=None), dict(poses=None), dict(tri_i8=None), dict(tri_row_stride=72 ** 3 - 1), dict(chunk=-1), dict(h=0), dict(w=32769)):
        assert call(_args(**kw), words=MO.min_words(129)) == INVALID, kw
        assert lib.gnbv_view_gain_slab(C.byref(_args(**kw)), 0, 0x4000, BIG, None) == INVALID, kw
    assert call(_args(), slab=-1) == INVALID
    need = lib.gnbv_view_gain_slab_workspace_bytes(2, 3, 72, 60, 80, 4)
    for ws, ws_bytes in ((None, BIG), (0x4000, need - 1), (0x4000, 0), (0x4008, BIG)):  # NULL, short, misaligned workspace
        assert call(_args(), ws=ws, ws_bytes=ws_bytes) == INVALID, (ws, ws_bytes)
    assert call(_args(), ub=None, hb=None) == INVALID                              # both outputs NULL
    for words in (0, -4, WORDS - 4, WORDS - 1, WORDS + 1, WORDS + 2, WORDS + 3):  # not a positive multiple of 4, or too small
        assert call(_args(), words=words) == INVALID, words
    assert call(_args(g=65, tri_row_stride=65 ** 3), words=8580) == INVALID       # ceil(274625 / 32) = 8583 -> 8584
    assert call(_args(g=128, tri_row_stride=128 ** 3), words=65532) == INVALID    # 128^3 / 32 = 65536
    for ub, hb in ((0x2004, 0x3000), (0x2000, 0x3008), (0x2001, None), (None, 0x300c)):
        assert call(_args(), ub=ub, hb=hb) == INVALID, (ub, hb)                   # not 16-byte aligned
    assert call(_args(n=65536, k=4096, g=2, tri_row_stride=8), words=8) == INVALID         # n k words = 2^31
    assert call(_args(n=512, k=64, g=128, tri_row_stride=128 ** 3), words=65536) == INVALID  # 2^31 at the flagship grid
    for ablate in (1, 2, 3):
        assert call(_args(ablate=ablate)) == INVALID, ablate


def test_operator_refuses_cpu_large_grids_large_masks_and_no_mask():
    from gennbv_amd import _lib
    from gennbv_amd.ops import gain_masks as GM
    assert issubclass(GM.ViewGainMasksSlab, GM.ViewGainMasks)
    assert GM.ViewGainMasksSlab.plan is GM.ViewGainMasks.plan and GM.ViewGainMasksSlab.plan_weighted is GM.ViewGainMasks.plan_weighted
    cfg = TaskConfig(camera_width=80, camera_height=60, grid_size=72)
    sc = S.make_scenes(2, 72, seed=1)
    with pytest.raises(_lib.GennbvHipError, match="GPU only"):
        GM.ViewGainMasksSlab(2, 4, cfg, sc.range_gt, sc.voxel_size, device="cpu")
    with pytest.raises(_lib.GennbvHipError, match="grid_size <= 128, got 129"):
        GM.ViewGainMasksSlab(2, 4, TaskConfig(camera_width=80, camera_height=60, grid_size=129), sc.range_gt, sc.voxel_size, device="cuda:0")
    with pytest.raises(_lib.GennbvHipError, match="grid_size <= 128, got 129"):
        GM.make_view_gain_masks(2, 4, TaskConfig(camera_width=80, camera_height=60, grid_size=129), sc.range_gt, sc.voxel_size, device="cuda:0")
    with pytest.raises(_lib.GennbvHipError, match="above max_bytes = 1000"):
        GM.ViewGainMasksSlab(2, 4, cfg, sc.range_gt, sc.voxel_size, device="cuda:0", max_bytes=1000)
    with pytest.raises(_lib.GennbvHipError, match="above max_bytes = 1000"):
        GM.make_view_gain_masks(2, 4, cfg, sc.range_gt, sc.voxel_size, device="cuda:0", max_bytes=1000, slab=5)
    for kw in (dict(words=WORDS - 4), dict(words=WORDS + 2), dict(hit=False, unknown=False)):
        with pytest.raises(_lib.GennbvHipError):
            GM.ViewGainMasksSlab(2, 4, cfg, sc.range_gt, sc.voxel_size, device="cuda:0", **kw)
    # the LDS operator still refuses grids above 64, and says where to go
    with pytest.raises(_lib.GennbvHipError, match="ViewGainMasksSlab / make_view_gain_masks"):
        GM.ViewGainMasks(2, 4, cfg, sc.range_gt, sc.voxel_size, device="cuda:0")


# ---------------------------------------------------------------------------
# The word-ownership rule (csrc/viewgain.hip, k_vg_slab<true> and k_vg_prep<true>), in integers.
#
# Slab sl of height s holds the row's bits [X0 g^2, X1 g^2), X0 = sl s, X1 = min(g, X0 + s).  Its LDS masks are biased by
# sh = X0 g^2 & 127, so LDS word i is row word 4 (X0 g^2 >> 7) + i and the slab's bits are [lo, hi) = [sh, sh + (X1 - X0) g^2) of
# the LDS mask; the last slab owns the row to the end of its last quad (hi = 128 nq).  LDS word i = bits [32 i, 32 i + 32):
#   outside [lo, hi)       another slab's word: not touched;
#   inside [lo, hi)        stored whole (as part of a 16-byte store where its whole quad is inside);
#   otherwise              shared with a neighbour: atomicOr of the slab's part into a word k_vg_prep<true> has zeroed.
# k_vg_prep<true> zeroes the word of every seam sl s g^2, 1 <= sl < nslab, that is not a multiple of 32, and the pad words
# [ceil(g^3 / 32), words).
# ---------------------------------------------------------------------------
def slab_plan(g, s, sl):
    """-> (first row word of the slab's LDS masks, sh, number of LDS words in use, whole LDS words [a, b), shared LDS words)."""
    gg = g * g
    x0, x1 = sl * s, min(g, sl * s + s)
    base, svox = x0 * gg, (x1 - x0) * gg
    sh = base & 127
    nq = (sh + svox + 127) >> 7
    lo, hi = sh, (nq * 128 if x1 == g else sh + svox)
    a, b = (lo + 31) // 32, hi // 32          # words inside [lo, hi)
    ta, tb = lo // 32, (hi + 31) // 32        # words that meet [lo, hi)
    shared = list(range(ta, tb)) if b <= a else list(range(ta, a)) + list(range(b, tb))  # met, but not inside
    return 4 * (base >> 7), sh, 4 * nq, (a, max(a, b)), shared


def zeroed_words(g, s, words):
    gg, nslab, row_words = g * g, (g + s - 1) // s, (g ** 3 + 31) // 32
    seams = {(sl * s * gg) >> 5 for sl in range(1, nslab) if (sl * s * gg) & 31}
    return seams | set(range(row_words, words))


def test_every_row_word_has_one_owner_or_two_sharers_and_the_zeroed_set_is_the_shared_set():
    for g in range(2, 129):
        row_words, words = (g ** 3 + 31) // 32, MO.min_words(g) + 4
        for s in range(1, g + 1):
            nslab = (g + s - 1) // s
            sharers, gaps, end = {}, set(), 0  # end: the row words below it are accounted for
            for sl in range(nslab):
                w0, sh, used, (a, b), shared = slab_plan(g, s, sl)
                assert 0 <= sh < 128 and (sh == 0 or (s * g * g) % 128 != 0)   # no bias, no extra LDS, where s g^2 % 128 == 0
                assert used * 32 >= sh + (min(g, sl * s + s) - sl * s) * g * g  # the LDS masks hold the biased slab
                assert used * 32 <= 4 * ((s * g * g + (127 if (s * g * g) % 128 else 0) + 127) // 128) * 32  # slab_lds_bytes(masks)
                assert w0 % 4 == 0 and w0 + b <= MO.min_words(g)             # 16-byte alignment; inside the shortest legal row
                assert len(shared) <= 2 and all(w0 + i < row_words for i in shared)
                for i in shared:
                    sharers.setdefault(w0 + i, []).append(sl)
                if b > a:  # the slab's whole words [w0 + a, w0 + b) follow the earlier slabs': no word is stored whole twice,
                    assert w0 + a >= end, (g, s, sl)  # and the words in between are stored whole by nobody
                    gaps |= set(range(end, w0 + a))
                    end = w0 + b
            # every word below row_words: one whole store, or none and its sharers (the last slab's last quad may reach into the
            # pad: zeros, as the prep's)
            gaps |= set(range(end, row_words))
            assert gaps == set(sharers), (g, s)
            for w, sls in sharers.items():
                # adjacent slabs; two of them, except where a whole slab is shorter than a word (g = 3, s = 1: 9 bits)
                assert sls == list(range(sls[0], sls[0] + len(sls))) and len(sls) >= 2, (g, s, w, sls)
                assert len(sls) == 2 or (g, s) == (3, 1), (g, s, w, sls)
            assert zeroed_words(g, s, words) == set(sharers) | set(range(row_words, words)), (g, s)


@pytest.mark.parametrize("g,s", [(65, 24), (33, 3), (127, 5), (128, 16), (100, 7), (3, 1), (5, 2), (72, 5), (128, 19)])
def test_slab_parts_assemble_into_the_directly_built_row(g, s):
    rng = np.random.RandomState(g * 131 + s)
    gg, g3, nslab = g * g, g ** 3, (g + s - 1) // s
    lins = np.unique(np.concatenate([rng.randint(0, g3, size=max(4, g3 // 7)), [0, g3 - 1],
                                     [sl * s * gg + d for sl in range(1, nslab) for d in (-1, 0) if 0 <= sl * s * gg + d < g3]]))
    for words in (MO.min_words(g), MO.min_words(g) + 8):
        want = MO.bits_of(lins, words)
        row = np.full(words, 0xFFFFFFFF, np.uint32)
        row[sorted(zeroed_words(g, s, words))] = 0           # k_vg_prep<true>
        for sl in rng.permutation(nslab):                    # the slab workgroups, in any order
            w0, sh, used, (a, b), shared = slab_plan(g, s, int(sl))
            x0, x1 = sl * s, min(g, sl * s + s)
            mine = lins[(lins >= x0 * gg) & (lins < x1 * gg)]
            lds = MO.bits_of(mine - x0 * gg + sh, used)      # slab-local voxel + sh
            row[w0 + a:w0 + b] = lds[a:b]
            for i in shared:
                row[w0 + i] |= lds[i]
        assert np.array_equal(row, want), np.argwhere(row != want)[:5].tolist()
