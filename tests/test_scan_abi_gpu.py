"""GPU: the scan set, the key sort and the accuracy scorer of csrc/scan.hip at their C ABI -- gnbv_scan_add_frame,
gnbv_scan_clear, gnbv_scan_export and gnbv_scan_score through ctypes on buffers the test places itself -- and
gnbv_chamfer_distance of csrc/chamfer.hip, the comparand of the scores.

Keys enter a set only through gnbv_scan_add_frame (the Morton layout of `keys` is not in the header and no test writes it): lattice
and point frames of tests/scan_abi_util.py, whose keys the numpy oracle computes with the bit-exact fp32 chain.  After every call
the counts, the flags and the export are compared with that oracle bit for bit, and the bytes around every buffer (the workspace,
exactly gnbv_scan_workspace_bytes long, included) must still hold their sentinel.

Every score is compared with
  1. 100 x oracle.chamfer_distance_ref (fp64 brute force) over the oracle's fp32 points and the GT as given, within
     8 * 2^-24 relative + 1e-30 absolute.  Derived, not measured (u = 2^-24): the pair value fmaf(dz,dz,fmaf(dy,dy,dx*dx)) on fp32
     differences is within (1+u)^5 of the true squared distance; a minimum and a sum of non-negative terms keep that relative
     bound; the fp64 sums add nothing visible; the fp32 cast and the fp32 x 100 add one u each: 7 u, rounded up to 8 u;
  2. gnbv_chamfer_distance over the exported points and the same GT, x 100.0f: at most 2 fp32 ulps (the header's statement).

Every case first asserts, from the oracle alone, that it reaches the regime its id names (scan_abi_util.check_regime;
tests/test_scan_abi_regimes_cpu.py runs the same assertions without a GPU)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import scan_abi_util as U
from tests.scan_abi_util import DEV, FILL, f32

pytestmark = pytest.mark.gpu
SENTINEL_F32 = np.frombuffer(bytes([FILL]) * 4, np.int32)[0]


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.int32)


def _add_all(call, oracle, frames, envs, where):
    """Every frame through gnbv_scan_add_frame; counts, flags and the export of `envs` against the oracle after every call."""
    for i, fr in enumerate(frames):
        assert call.add(fr) == 0, (where, i)
        oracle.add(fr)
        call.check_set(oracle, envs, f"{where}: add {i}")


def _score(call, oracle, clouds, mask, where):
    """One gnbv_scan_score: exactly the envs of the header's predicate get scored = 1 and an accuracy that passes both comparisons;
    accuracy and scored of every other env keep their bits.  Returns the scored envs."""
    mask = np.asarray(mask, np.uint8)
    scored0, acc0 = call.read_scored().copy(), _bits(call.read_accuracy()).copy()
    assert call.score(mask) == 0, where
    active = [e for e in range(call.n) if mask[e] and not scored0[e] and oracle.counts[e] > 0 and oracle.flags[e] == 0]
    want = scored0.copy()
    want[active] = 1
    assert np.array_equal(call.read_scored(), want), (where, "scored")
    rest = np.setdiff1d(np.arange(call.n), active)
    assert np.array_equal(_bits(call.read_accuracy())[rest], acc0[rest]), (where, "accuracy of an env that was not scored changed")
    call.check_scores(oracle, clouds, active, where)
    assert call.intact(), f"{where}: bytes outside a buffer were written"
    return active


def _ascending(call, oracle, envs):
    """The header: score sorts the key list of the scored envs in place."""
    for e in envs:
        k = call.keys_row(e)[:int(oracle.counts[e])]
        assert np.all(k[1:] > k[:-1]), f"env {e}: the key list is not sorted"


# ---------------------------------------------------------------------------
# the set
# ---------------------------------------------------------------------------
def test_cap64_fill_wrap():
    """capacity 64 (cap >> 6 == 1: a key's first slot is its low six code bits), 64 keys = 3 mod 4 on every axis in two frames of
    32: all share first slot 63, every probe wraps past the last slot, and the table ends exactly full."""
    U.check_regime("cap64-fill-wrap")
    c = U.case("cap64-fill-wrap")
    call, o = U.ScanCall(c.n, c.cap, U.pack_gt(c.clouds)), U.SetOracle(c.n, c.cap)
    _add_all(call, o, c.frames, [0, 1], "fill")
    assert call.read_counts().tolist() == [64, 32] and call.read_flags().tolist() == [0, 0]
    assert not (call.table_row(0) == np.uint64(2 ** 64 - 1)).any()  # no empty slot left in env 0
    before = call.snapshot()
    _add_all(call, o, c.frames, [0, 1], "the same frames again")
    assert call.snapshot() == before, "re-adding keys the set holds changed a buffer"
    assert _score(call, o, c.clouds, [1, 1], "full table") == [0, 1]
    call.check_set(o, [0, 1], "after the score")
    # one more distinct key per env: env 0 is full -> overflow flag, count stays 64; env 1 takes it
    rows = [call.table_row(0).copy(), call.keys_row(0).copy()]
    assert call.add(c.extra) == 0
    o.add(c.extra)
    assert o.counts.tolist() == [64, 33] and o.flags.tolist() == [U.FLAG_OVERFLOW, 0]
    call.check_set(o, [1], "one key too many")  # (no export of the flagged env)
    assert np.array_equal(call.table_row(0), rows[0]) and np.array_equal(call.keys_row(0), rows[1])
    call.scored.write(np.zeros(2, np.int32))
    assert _score(call, o, c.clouds, [1, 1], "a flagged env is not scored") == [1]


def test_load_factor_one():
    """capacity 4096 and 4096 distinct keys per env over two 32 x 64 lattice frames (load factor 1 on the last key), then a frame
    that repeats half of them."""
    U.check_regime("load-factor-one")
    c = U.case("load-factor-one")
    call, o = U.ScanCall(c.n, c.cap), U.SetOracle(c.n, c.cap)
    _add_all(call, o, c.frames, [0, 1], "load factor one")
    assert call.read_counts().tolist() == [4096, 4096] and call.read_flags().tolist() == [0, 0]
    for e in range(2):
        assert not (call.table_row(e) == np.uint64(2 ** 64 - 1)).any()


@pytest.mark.parametrize("sub", ["16x16-one-key", "16x16-two-keys", "5x13-two-keys", "1x1"])
def test_duplicates_in_a_wave(sub):
    """Every lane of a wave on one key (count 1), two keys alternating lane by lane (count 2), 65 pixels (lanes >= h w in the
    ballots of the second wave) and a single pixel."""
    U.check_regime("duplicates-in-a-wave")
    c = U.case("duplicates-in-a-wave")
    call, o = U.ScanCall(c.n, c.cap), U.SetOracle(c.n, c.cap)
    _add_all(call, o, c.subs[sub] * 2, [0, 1, 2], sub)
    assert call.read_counts().tolist() == c.finals[sub].counts.tolist()


def test_key_range_edges():
    """k = +-(2^20 - 1) on every axis is accepted and exported as fp32(+-1048575) * 0.01f; k = +-2^20, NaN and +-inf are refused with
    flag bit 1 and count 0; a frame with one pixel of each kind adds the good key and sets the flag."""
    U.check_regime("key-range-edges")
    c = U.case("key-range-edges")
    call, o = U.ScanCall(c.n, c.cap), U.SetOracle(c.n, c.cap)
    _add_all(call, o, c.frames, c.accepted, "edges")
    for e in c.accepted:
        assert call.export(e).tobytes() == (c.want[e].astype(f32) * f32(0.01)).astype(f32).reshape(1, 3).tobytes(), e
    assert call.read_counts()[c.refused].tolist() == [0] * 7 and call.read_flags()[c.refused].tolist() == [U.FLAG_RANGE] * 7
    assert call.read_counts()[15] == 1 and call.read_flags()[15] == U.FLAG_RANGE
    for e in c.refused:
        assert (call.table_row(e) == np.uint64(2 ** 64 - 1)).all(), e


def test_masked_clear():
    """n = 5, mask [1, 0, 1, 0, 0]: table and keys rows and the counts of the other envs are byte-identical, the masked table rows
    are all-ones bytes with count 0, a flag set before the clear is still set, and re-adding gives the oracle's fresh set."""
    U.check_regime("masked-clear")
    c = U.case("masked-clear")
    call, o = U.ScanCall(c.n, c.cap), U.SetOracle(c.n, c.cap)
    _add_all(call, o, c.before, range(c.n), "before the clear")
    assert call.read_flags().tolist() == [2, 2, 0, 0, 0]
    table, keys, counts = call.table.read(np.uint64, (c.n, c.cap)).copy(), call.keys.read(np.uint64, (c.n, c.cap)).copy(), call.read_counts().copy()
    assert call.clear(c.mask) == 0
    o.clear(c.mask)
    t2, k2 = call.table.read(np.uint64, (c.n, c.cap)), call.keys.read(np.uint64, (c.n, c.cap))
    for e in range(c.n):
        if c.mask[e]:
            assert (t2[e] == np.uint64(2 ** 64 - 1)).all() and call.read_counts()[e] == 0, e
        else:
            assert np.array_equal(t2[e], table[e]) and np.array_equal(k2[e], keys[e]) and call.read_counts()[e] == counts[e], e
    assert call.read_flags().tolist() == [2, 2, 0, 0, 0], "flags are kept by clear"
    call.check_set(o, range(c.n), "after the clear")
    _add_all(call, o, c.after, range(c.n), "re-adding")
    assert call.read_counts().tolist() == [40, 64 + 41, 42, 64 + 43, 64 + 44]


def test_clear_grid_stride():
    """n = 1024 (4 blocks per env) and capacity 4096: 2048 uint4 per env on 1024 threads, the second trip of k_scan_clear's loop."""
    info = U.check_regime("clear-grid-stride")
    assert info["trips"] == 2
    c = U.case("clear-grid-stride")
    call = U.ScanCall(c.n, c.cap)
    call.table.data.fill_(FILL)
    call.counts.write(np.full(c.n, 7, np.int32))
    call.flags.write(np.full(c.n, 3, np.int32))
    assert call.clear(np.ones(c.n, np.uint8)) == 0
    for e in (0, 1, c.n - 1):
        assert (call.table_row(e) == np.uint64(2 ** 64 - 1)).all(), e
    assert bool((call.table.data == 0xFF).all()) and bool((call.keys.data == FILL).all())
    assert not call.read_counts().any() and (call.read_flags() == 3).all()
    assert call.intact()


# ---------------------------------------------------------------------------
# the sort (through export and score)
# ---------------------------------------------------------------------------
def _sort_case(cid, export_every_call=True):
    U.check_regime(cid)
    c = U.case(cid)
    call, o = U.ScanCall(c.n, c.cap, U.pack_gt(c.clouds)), U.SetOracle(c.n, c.cap)
    envs = getattr(c, "loaded", range(c.n))
    _add_all(call, o, c.frames, envs, cid)
    assert o.counts.tolist() == c.final.counts.tolist()
    active = _score(call, o, c.clouds, np.ones(c.n, np.uint8), cid)
    assert active == [e for e in range(c.n) if o.counts[e] > 0]
    _ascending(call, o, active)
    call.check_set(o, envs, f"{cid}: after the score")  # the sorted list still holds the same set
    return c, call, o


def test_tile_edges():
    """Six envs in one call with 1, 8, 2047, 2048, 2049 and 0 keys (kSortTile = 2048): every env sorts its own count."""
    _, call, _ = _sort_case("tile-edges")
    assert call.read_scored().tolist() == [1, 1, 1, 1, 1, 0]
    assert _bits(call.read_accuracy())[5] == SENTINEL_F32


def test_scan_carry():
    """32 768 keys (16 tiles: exactly one 256-entry chunk of k_radix_scan) and 34 817 keys (18 tiles: a second chunk, with carry)."""
    _sort_case("scan-carry")


def test_tiles_over_blocks():
    """n = 1024: 4 blocks per env; envs 0 and 511 sort 5 tiles on 4 blocks (a second trip of the tile loops of k_radix_hist and
    k_radix_scatter), env 1023 two tiles; every other env is empty and keeps the sentinel in `accuracy`."""
    c, call, _ = _sort_case("tiles-over-blocks")
    scored, acc = call.read_scored(), _bits(call.read_accuracy())
    rest = np.setdiff1d(np.arange(c.n), c.loaded)
    assert scored[c.loaded].tolist() == [1, 1, 1] and not scored[rest].any() and (acc[rest] == SENTINEL_F32).all()


def test_insertion_order():
    """The same frames in two orders into two sets: equal exports, equal accuracy bits.  Then score, add a frame, zero `scored` and
    score again: the list was sorted in place and appended to, and the result is the oracle's of the union."""
    U.check_regime("insertion-order")
    c = U.case("insertion-order")
    g = U.pack_gt(c.clouds)
    calls = []
    for order in c.orders:
        call, o = U.ScanCall(c.n, c.cap, g), U.SetOracle(c.n, c.cap)
        _add_all(call, o, [c.frames[i] for i in order], range(c.n), f"order {order}")
        calls.append((call, o))
    (a, oa), (b, ob) = calls
    for e in range(c.n):
        assert a.export(e).tobytes() == b.export(e).tobytes()
        assert not np.array_equal(a.keys_row(e)[:oa.counts[e]], b.keys_row(e)[:ob.counts[e]])  # (the append orders did differ)
    for call, o in calls:
        assert _score(call, o, c.clouds, [1, 1], "three frames") == [0, 1]
    assert _bits(a.read_accuracy()).tolist() == _bits(b.read_accuracy()).tolist()
    first = _bits(a.read_accuracy()).copy()
    for call, o in calls:
        _add_all(call, o, c.frames[3:], range(c.n), "a frame after the score")
        assert o.counts.tolist() == c.final4.counts.tolist()
        call.scored.write(np.zeros(c.n, np.int32))
        assert _score(call, o, c.clouds, [1, 1], "four frames") == [0, 1]
        _ascending(call, o, [0, 1])
    assert _bits(a.read_accuracy()).tolist() == _bits(b.read_accuracy()).tolist()
    assert (_bits(a.read_accuracy()) != first).all()


# ---------------------------------------------------------------------------
# the trees and the minima
# ---------------------------------------------------------------------------
def test_tree_sizes():
    """Scan counts 1, 32, 33, 64, 65, 1024, 1025 (P from 1 to 2 at 32 / 33; 32 * 2^j and 32 * 2^j + 1, where half the heap is empty
    boxes) against GT clouds of 1, 32, 33, 1025, 1, 32, 33 points, seven envs in one call."""
    _sort_case("tree-sizes")


@pytest.mark.parametrize("packer", ["numpy", "gt_tree"])
def test_degenerate_gt(packer):
    """GT = the env's own points (accuracy exactly 0.0f); 100 identical GT points (_gt_tree's clamp(hi - lo, min=1e-30)); GT on one
    axis-parallel line through lattice points (zero-extent boxes, lb == 0: the !(lb > 2^-100) path of nn_tree); GT = a 2049-key set
    +- 0.005 on each axis (six tied nearest neighbours, most in different leaves); GT 40 m from the scan."""
    U.check_regime("degenerate-gt")
    c = U.case("degenerate-gt")
    g = U.pack_gt(c.clouds) if packer == "numpy" else U.pack_from_gt_tree(c.clouds, DEV)
    U.check_gt_invariants(g, c.clouds)
    call, o = U.ScanCall(c.n, c.cap, g), U.SetOracle(c.n, c.cap)
    _add_all(call, o, c.frames, range(c.n), "degenerate-gt")
    assert _score(call, o, c.clouds, np.ones(c.n, np.uint8), f"degenerate-gt/{packer}") == list(range(c.n))
    assert _bits(call.read_accuracy())[0] == 0, "a set scored against its own points is not exactly 0.0f"


def test_gt_order():
    """The same clouds packed in the given order (numpy), in a seeded permutation with a heap one level taller (orig maps back) and
    by ScanAccumulator._gt_tree: the accuracies agree within 2 ulps and each passes the oracle check; _gt_tree's heap satisfies the
    header's invariants."""
    U.check_regime("gt-order")
    c = U.case("gt-order")
    packs = {"given": U.pack_gt(c.clouds), "permuted": U.pack_gt(c.clouds, c.perms, extra_levels=1), "gt_tree": U.pack_from_gt_tree(c.clouds, DEV)}
    call, o = U.ScanCall(c.n, c.cap), U.SetOracle(c.n, c.cap)
    _add_all(call, o, c.frames, range(c.n), "gt-order")
    acc = {}
    for name, g in packs.items():
        U.check_gt_invariants(g, c.clouds)
        call.use_gt(g)
        call.scored.write(np.zeros(c.n, np.int32))
        assert _score(call, o, c.clouds, np.ones(c.n, np.uint8), f"gt-order/{name}") == list(range(c.n))
        acc[name] = call.read_accuracy().copy()
    assert not np.array_equal(packs["gt_tree"].orig, packs["given"].orig)
    for e in range(c.n):
        for name in ("permuted", "gt_tree"):
            assert U.ulps(acc["given"][e], acc[name][e]) <= 2, (e, name, acc["given"][e], acc[name][e])


def test_mask_semantics():
    """One call, six envs: mask 0, already scored, empty and flagged envs keep their accuracy bits, `scored` and keys row; the two
    active envs are scored."""
    U.check_regime("mask-semantics")
    c = U.case("mask-semantics")
    call, o = U.ScanCall(c.n, c.cap, U.pack_gt(c.clouds)), U.SetOracle(c.n, c.cap)
    _add_all(call, o, c.frames, range(c.n), "mask-semantics")
    scored = np.zeros(c.n, np.int32)
    scored[c.prescored] = 1
    call.scored.write(scored)
    keys, table = call.keys.read(np.uint64, (c.n, c.cap)).copy(), call.table.snapshot()
    assert _score(call, o, c.clouds, c.mask, "mask-semantics") == c.active
    assert call.read_scored().tolist() == [1, 0, 1, 0, 0, 1]
    assert (_bits(call.read_accuracy())[c.inactive] == SENTINEL_F32).all()
    k2 = call.keys.read(np.uint64, (c.n, c.cap))
    for e in c.inactive:
        assert np.array_equal(k2[e], keys[e]), f"the keys row of env {e} changed"
    assert call.table.snapshot() == table and call.read_counts().tolist() == o.counts.tolist() and call.read_flags().tolist() == o.flags.tolist()
    _ascending(call, o, c.active)


def test_refusals():
    """Argument checks that launch nothing: each returns non-zero and changes no buffer, sentinels included.  Every pointer a check
    does not refuse is a valid device pointer."""
    n, cap = 2, 128
    fr = U.lattice_frame(U.base_translations(n), 8, 8)
    o = U.final_oracle(n, cap, [fr])
    clouds = [U.gt_near(o.points(e), 10, e) for e in range(n)]
    call = U.ScanCall(n, cap, U.pack_gt(clouds))
    L = call.L
    assert call.add(fr) == 0
    ones = np.ones(n, np.uint8)
    call.mask.write(ones)
    out = U.Buf(64 * 12)
    frame_bufs = list(call.frame_bufs)
    before = call.snapshot(ws=True) + [out.snapshot()]
    s, g = call.set, call.gt.struct
    cap96 = L.GnbvScanSet(n, 96, s.table, s.keys, s.counts, s.flags)
    gt_n = L.GnbvScanGt(n + 1, g.num_points, g.pt_start, g.pts, g.orig, g.node_start, g.pow2, g.nodes)
    gt_0 = L.GnbvScanGt(n, 0, g.pt_start, g.pts, g.orig, g.node_start, g.pow2, g.nodes)
    kinv = (C.c_float * 9)(*fr.kinv.reshape(-1).tolist())
    refused = {
        "score: workspace one byte short": lambda: call.score(ones, ws_bytes=call.ws_bytes - 1),
        "score: workspace pointer + 128": lambda: call.score(ones, ws_ptr=call.ws.ptr + 128),
        "score: capacity 96": lambda: call.score(ones, set_=cap96),
        "score: gt->n != set->n": lambda: call.score(ones, gt=gt_n),
        "score: num_points == 0": lambda: call.score(ones, gt=gt_0),
        "score: NULL mask": lambda: call.score(ones, null_mask=True),
        "clear: NULL mask": lambda: call.clear(ones, null_mask=True),
        "clear: capacity 96": lambda: call.clear(ones, set_=cap96),
        "add_frame: capacity 96": lambda: call.lib.gnbv_scan_add_frame(C.byref(cap96), frame_bufs[0].ptr, frame_bufs[1].ptr, frame_bufs[2].ptr,
                                                                       kinv, fr.h, fr.w, U.SENSE, None),
        "export: env == n": lambda: call.export_raw(n, out),
        "export: env == -1": lambda: call.export_raw(-1, out),
        "export: capacity 96": lambda: call.export_raw(0, out, set_=cap96),
        "export: workspace one byte short": lambda: call.export_raw(0, out, ws_bytes=call.xws_bytes - 1),
        "export: workspace pointer + 128": lambda: call.export_raw(0, out, ws_ptr=call.xws.ptr + 128),
    }
    for name, f in refused.items():
        assert f() != 0, name
        torch.cuda.synchronize()
        assert call.snapshot(ws=True) + [out.snapshot()] == before, f"{name}: a refused call wrote"
    # and the same arguments without the fault go through
    assert call.export_raw(0, out) == 0 and out.read(f32, (64, 3)).tobytes() == o.points(0).tobytes()
    assert _score(call, o, clouds, ones, "after the refusals") == [0, 1]


# ---------------------------------------------------------------------------
# gnbv_chamfer_distance, the comparand
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", U.CHAMFER_SHAPES)
def test_chamfer_distance_shapes(n, m):
    """Around kTile = 1024 reference points per LDS tile and 1024 queries per workgroup, against the fp64 brute force at the derived
    bound: without the x 100 it is 6 u; checked at the same 8 * 2^-24 relative + 1e-30."""
    x, y = U.chamfer_clouds(n, m)
    U.assert_close_to_ref(U.device_chamfer(x, y), U.ref_chamfer(x, y), f"chamfer {n} x {m}")
    U.assert_close_to_ref(U.device_chamfer(y, x), U.ref_chamfer(x, y), f"chamfer {m} x {n}")


def test_chamfer_distance_workspace_refusals():
    x, y = U.chamfer_clouds(5, 2049)
    assert U.device_chamfer(x, y, ws_short=1) != 0
    assert U.device_chamfer(x, y, ws_offset=8) != 0
