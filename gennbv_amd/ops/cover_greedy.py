"""What ViewPool and ViewGainMasks share of greedy set cover (csrc/covergreedy.hip gnbv_cover_greedy, gnbv_cover_greedy_w): the
argument checks, the argument struct and its launch, and the outputs kept per `rounds`.  `who` names the calling class and method
in every message; every check comes before any launch."""
from __future__ import annotations

import ctypes as C

import torch

from .. import _lib

MAX_ROUNDS = 4096


def check_rounds(who: str, rounds) -> int:
    rounds = int(rounds)
    if not 1 <= rounds <= MAX_ROUNDS:
        raise _lib.GennbvHipError(f"{who}: rounds in 1..{MAX_ROUNDS}, got {rounds}")
    return rounds


def _check_rows(who: str, what: str, t, dtype, shape):
    if t is None:
        return None
    _lib.require_cuda(t)
    if t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
        raise _lib.GennbvHipError(f"{who}: {what} must be contiguous {str(dtype)[6:]} {list(shape)}, got {t.dtype} {tuple(t.shape)}")
    return t


def check_contact(who: str, contact, n: int, k: int):
    return _check_rows(who, "contact", contact, torch.uint8, (n, k))


def check_covered(who: str, covered_bits, n: int, words: int):
    return _check_rows(who, "covered_bits", covered_bits, torch.int32, (n, words))


class CoverGreedy:
    """One entry point's argument struct for n envs x k candidates x `words` words per row, and its outputs per `rounds`.
    planes = 0: gnbv_cover_greedy, masks / covered rows are single tensors; planes >= 1: gnbv_cover_greedy_w, they are one tensor
    per plane."""

    def __init__(self, lib, device, n: int, k: int, words: int, planes: int = 0):
        self.lib, self.device, self.n, self.k, self.words, self.planes = lib, device, n, k, words, planes
        a = _lib.GnbvCoverGreedyW() if planes else _lib.GnbvCoverGreedy()
        a.n, a.k, a.words = n, k, words
        if planes:
            a.planes = planes
        self._args = a
        self._outputs = {}

    def outputs(self, rounds: int):
        """(choice [N,T], gain [N,T], covered, plane_gain) int32, allocated on the first call with this `rounds` and reused:
        covered [N, words] and None, or with planes a tuple of one row per plane and [N,T,planes]."""
        if rounds not in self._outputs:
            new = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=self.device)
            n, p = self.n, self.planes
            self._outputs[rounds] = (new(n, rounds), new(n, rounds), tuple(new(n, self.words) for _ in range(p)) if p else new(n, self.words),
                                     new(n, rounds, p) if p else None)
        return self._outputs[rounds]

    def launch(self, rounds, masks, covered_in, contact, choice, gain, covered_out, gains0=None, ub=None, lazy=True, weights=None,
               plane_gain=None):
        a = self._args
        a.rounds, a.contact, a.lazy = int(rounds), _lib.ptr(contact), int(bool(lazy))
        a.choice, a.gain, a.gains0, a.ub = choice.data_ptr(), gain.data_ptr(), _lib.ptr(gains0), _lib.ptr(ub)
        if self.planes:
            for p in range(self.planes):
                a.weight[p], a.mask_bits[p] = weights[p], masks[p].data_ptr()
                a.covered_in[p] = None if covered_in is None else _lib.ptr(covered_in[p])
                a.covered_out[p] = None if covered_out is None else _lib.ptr(covered_out[p])
            a.plane_gain = _lib.ptr(plane_gain)
            _lib.check(self.lib.gnbv_cover_greedy_w(C.byref(a), _lib.stream_ptr(self.device)), "gnbv_cover_greedy_w")
        else:
            a.mask_bits, a.covered_in, a.covered_out = masks.data_ptr(), _lib.ptr(covered_in), _lib.ptr(covered_out)
            _lib.check(self.lib.gnbv_cover_greedy(C.byref(a), _lib.stream_ptr(self.device)), "gnbv_cover_greedy")
