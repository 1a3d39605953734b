"""ViewGainMasks: the view gain that keeps what it counts, and greedy set cover on it  (csrc/viewgain.hip gnbv_view_gain_masks
and gnbv_view_gain_slab_masks, csrc/covergreedy.hip gnbv_cover_greedy).

ViewGain reduces, per candidate, the set of unknown voxels its rays would cross to three integers; two candidates that would see
the SAME unknown voxels both look good.  ViewGainMasks runs the same kernel and also stores the two sets as bit masks --
`unknown_bits` (every ray) and `hit_bits` (the rays that meet a surface), int32 [N, K, words] in the layout of the updater's
scanned_bits and of gnbv_cover_greedy (bit lin & 31 of word lin >> 5, lin = (x G + y) G + z) -- so that `plan(T)` can pick T views
that add DIFFERENT voxels: the classic greedy set cover, on the map the pilot holds and nothing else; `plan_weighted(T, weights)`
is the same under the greedy planners' score w_unknown * new unknown voxels + w_hit * new hit voxels, on both masks at once
(csrc/covergreedy.hip gnbv_cover_greedy_w).  Integers with one right
answer (include/gennbv_hip.h has the exact definitions).  Outputs are preallocated and reused: a result is valid until the next
call of the same method.  No host synchronisation in either call.  GPU only, no CPU fallback.

ViewGainMasks stores the masks from the LDS of the one-launch kernel (grid_size <= 64); ViewGainMasksSlab computes the same rows
for grid_size <= 128 through gnbv_view_gain_slab_masks (the slab kernels of ViewGainSlab, each slab storing its part of a row)
with a preallocated workspace, and plans on them with the same `plan` / `plan_weighted`; make_view_gain_masks picks.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from .. import _lib
from ..env.config import TaskConfig
from .cover_greedy import CoverGreedy, check_contact, check_covered, check_rounds
from .view_gain import MAX_GRID, MAX_GRID_SLAB, ViewGain, slab_workspace


def plan_weights(weights, words: int):
    """(w_unknown, w_hit) as two ints, or a GennbvHipError with the reason: what gnbv_cover_greedy_w refuses for its weights."""
    try:
        w = tuple(int(x) for x in weights)
        whole = all(x == y for x, y in zip(w, weights))
    except (TypeError, ValueError):
        w, whole = (), False
    if len(w) != 2 or not whole:
        raise _lib.GennbvHipError(f"ViewGainMasks.plan_weighted: weights must be two integers (w_unknown, w_hit), got {weights!r}")
    if min(w) < 0:
        raise _lib.GennbvHipError(f"ViewGainMasks.plan_weighted: weights must be >= 0, got {w}")
    if sum(w) * 32 * int(words) > 2 ** 31 - 1:
        raise _lib.GennbvHipError(f"ViewGainMasks.plan_weighted: (w_unknown + w_hit) * 32 * words = {sum(w) * 32 * int(words)} exceeds "
                                  f"2^31 - 1 (weights {w}, {int(words)} words): a score would not fit in int32")
    return w


class ViewGainMasks(ViewGain):
    def __init__(self, num_envs: int, k: int, cfg: TaskConfig, range_gt: torch.Tensor, voxel_size: torch.Tensor,
                 inv_intrinsics: Optional[torch.Tensor] = None, stride: int = 4, range_m: Optional[float] = None,
                 device="cuda:0", hit: bool = True, unknown: bool = True, words: Optional[int] = None, max_bytes: int = 8 << 30,
                 with_c2w: bool = False, chunk: int = 0):
        """ViewGain's arguments, plus: `hit` / `unknown` choose the masks to keep (at least one); `words` is the row length
        (None: gnbv_grid_bit_words(G), the updater's; any multiple of 4 that holds G^3 bits); `max_bytes` caps the masks."""
        g, name = int(cfg.grid_size), type(self).__name__
        if g > self._max_grid:
            raise _lib.GennbvHipError(f"{name}: grid_size <= {self._max_grid}, got {g}" + (
                " (the masks are stored from the LDS of the one-launch kernel; above, the slab kernels store them slab by slab: "
                f"ViewGainMasksSlab / make_view_gain_masks go up to {MAX_GRID_SLAB})" if self._max_grid == MAX_GRID else ""))
        if not (hit or unknown):
            raise _lib.GennbvHipError(f"{name}: at least one of hit, unknown")
        if torch.device(device).type != "cuda":
            raise _lib.GennbvHipError(f"{name} runs on the GPU only (no CPU fallback)")
        lib = _lib.load()
        n, k = int(num_envs), int(k)
        self.words = int(lib.gnbv_grid_bit_words(g)) if words is None else int(words)
        if self.words < 1 or self.words % 4 or self.words * 32 < g ** 3:
            raise _lib.GennbvHipError(f"{name}: words must be a multiple of 4 that holds {g}^3 bits, got {self.words}")
        kept = int(bool(hit)) + int(bool(unknown))
        nbytes = kept * n * k * self.words * 4
        if nbytes > int(max_bytes):
            raise _lib.GennbvHipError(f"{name}: the {kept} masks of {n} envs x {k} views x {self.words} words take {nbytes} "
                                      f"bytes, above max_bytes = {int(max_bytes)}")
        if n * k * self.words > 2 ** 31 - 1:
            raise _lib.GennbvHipError(f"{name}: {n} envs x {k} views x {self.words} words exceed 2^31 - 1 words")
        super().__init__(n, k, cfg, range_gt, voxel_size, inv_intrinsics, stride, range_m, device, with_c2w, chunk)
        dev = self.device
        self.unknown_bits = torch.empty(n, k, self.words, dtype=torch.int32, device=dev) if unknown else None
        self.hit_bits = torch.empty(n, k, self.words, dtype=torch.int32, device=dev) if hit else None
        self.gains0 = torch.empty(n, k, dtype=torch.int32, device=dev)
        self.plane_gain = None
        self._cg = CoverGreedy(lib, dev, n, k, self.words)  # plan's outputs, apart from ...
        self._cgw = CoverGreedy(lib, dev, n, k, self.words, planes=2)  # ... plan_weighted's

    def _launch(self, a):
        _lib.check(self.lib.gnbv_view_gain_masks(C.byref(a), self.words, _lib.ptr(self.unknown_bits), _lib.ptr(self.hit_bits),
                                                 _lib.stream_ptr(self.device)), "gnbv_view_gain_masks")

    def plan(self, rounds: int, which: str = "hit", contact: Optional[torch.Tensor] = None, covered_bits: Optional[torch.Tensor] = None,
             lazy: bool = True):
        """Greedy set cover over the `which` mask ("hit" | "unknown") of the last call: `rounds` views, each the candidate that
        adds the most voxels no earlier round covers, starting from covered_bits [N, words] int32 (None: nothing covered; not
        modified) -> (choice [N,T], gain [N,T], covered [N, words]) int32.  `contact` uint8 [N,K]: non-zero candidates are never
        chosen unless all of an env's are (then candidate 0).  `gains0` [N,K] holds round 0's gain of every candidate.  One
        gnbv_cover_greedy launch; `lazy` changes the work, not the result."""
        rounds = check_rounds("ViewGainMasks.plan", rounds)
        if which not in ("hit", "unknown"):
            raise _lib.GennbvHipError(f"ViewGainMasks.plan: which must be 'hit' or 'unknown', got {which!r}")
        masks = self.hit_bits if which == "hit" else self.unknown_bits
        if masks is None:
            raise _lib.GennbvHipError(f"ViewGainMasks.plan: the {which} mask is not kept ({which}=False)")
        check_contact("ViewGainMasks.plan", contact, self.num_envs, self.k)
        check_covered("ViewGainMasks.plan", covered_bits, self.num_envs, self.words)
        choice, gain, covered, _ = self._cg.outputs(rounds)
        self._cg.launch(rounds, masks, covered_bits, contact, choice, gain, covered, self.gains0, None, lazy)
        return choice, gain, covered

    def plan_weighted(self, rounds: int, weights=(1, 4), contact: Optional[torch.Tensor] = None, covered_bits=None, lazy: bool = True):
        """Greedy set cover on BOTH masks of the last call under the score of eval.baselines.choose: each round takes the
        candidate with the largest w_unknown * |new voxels of unknown_bits| + w_hit * |new voxels of hit_bits|, against two
        covered sets that grow together (plane 0 = unknown_bits, plane 1 = hit_bits; weights = (w_unknown, w_hit), ints >= 0)
        -> (choice [N,T], gain [N,T] the weighted score, (covered_unknown, covered_hit) [N, words] each) int32.
        `covered_bits`: None, or a pair of contiguous int32 [N, words] (unknown, hit; not modified).  `contact` as in `plan`.
        `plane_gain` int32 [N,T,2] holds the winners' gains per mask, `gains0` [N,K] the weighted round-0 score of every
        candidate.  Outputs are cached per `rounds`, apart from `plan`'s.  One gnbv_cover_greedy_w launch, no host
        synchronisation; `lazy` changes the work, not the result."""
        rounds = check_rounds("ViewGainMasks.plan_weighted", rounds)
        for name, masks in (("unknown", self.unknown_bits), ("hit", self.hit_bits)):
            if masks is None:
                raise _lib.GennbvHipError(f"ViewGainMasks.plan_weighted needs both masks: the {name} mask is not kept ({name}=False)")
        w = plan_weights(weights, self.words)
        check_contact("ViewGainMasks.plan_weighted", contact, self.num_envs, self.k)
        if covered_bits is not None:
            if not isinstance(covered_bits, (tuple, list)) or len(covered_bits) != 2:
                raise _lib.GennbvHipError("ViewGainMasks.plan_weighted: covered_bits must be None or a pair (unknown, hit)")
            for cb in covered_bits:
                check_covered("ViewGainMasks.plan_weighted", cb, self.num_envs, self.words)
        choice, gain, covered, self.plane_gain = self._cgw.outputs(rounds)
        self._cgw.launch(rounds, (self.unknown_bits, self.hit_bits), covered_bits, contact, choice, gain, covered, self.gains0, None, lazy,
                         weights=w, plane_gain=self.plane_gain)
        return choice, gain, covered


class ViewGainMasksSlab(ViewGainMasks):
    """The same operator for grid_size <= 128 (gnbv_view_gain_slab_masks): ViewGainMasks' arguments plus `slab`, the x-planes per
    slab (0 = chosen from the grid size; any height gives the same rows and integers).  `unknown_bits`, `hit_bits`, `words`,
    `max_bytes`, `gains0`, `plan`, `plan_weighted` and `plane_gain` are ViewGainMasks'; the workspace (ViewGainSlab's) is
    allocated once, here.  Sizes: at 128^3 a row is 65 536 words = 256 KiB, so 64 envs x K = 32 x both masks take 1 GiB and
    512 envs x 32 x both exactly the default `max_bytes` of 8 GiB (n k words = 2^30 words per mask, within the 2^31 - 1 limit);
    keep one mask (hit=False / unknown=False) to halve it."""
    _max_grid = MAX_GRID_SLAB

    def __init__(self, num_envs: int, k: int, cfg: TaskConfig, range_gt: torch.Tensor, voxel_size: torch.Tensor,
                 inv_intrinsics: Optional[torch.Tensor] = None, stride: int = 4, range_m: Optional[float] = None,
                 device="cuda:0", hit: bool = True, unknown: bool = True, words: Optional[int] = None, max_bytes: int = 8 << 30,
                 with_c2w: bool = False, chunk: int = 0, slab: int = 0):
        super().__init__(num_envs, k, cfg, range_gt, voxel_size, inv_intrinsics, stride, range_m, device, hit, unknown, words,
                         max_bytes, with_c2w, chunk)
        self.slab = int(slab)
        slab_workspace(self, "ViewGainMasksSlab")

    def _launch(self, a):
        _lib.check(self.lib.gnbv_view_gain_slab_masks(C.byref(a), self.slab, self.workspace.data_ptr(), self.workspace_bytes, self.words,
                                                      _lib.ptr(self.unknown_bits), _lib.ptr(self.hit_bits),
                                                      _lib.stream_ptr(self.device)), "gnbv_view_gain_slab_masks")


def make_view_gain_masks(num_envs: int, k: int, cfg: TaskConfig, *args, **kwargs) -> ViewGainMasks:
    """ViewGainMasks for grid_size <= 64 (one launch, the grid in LDS), ViewGainMasksSlab above; `slab` is passed to the latter
    only."""
    if int(cfg.grid_size) <= MAX_GRID:
        kwargs.pop("slab", None)
        return ViewGainMasks(num_envs, k, cfg, *args, **kwargs)
    return ViewGainMasksSlab(num_envs, k, cfg, *args, **kwargs)
