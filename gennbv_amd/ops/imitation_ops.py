"""Host side of the soft-target imitation loss (gennbv_amd/csrc/imitation.hip)."""
from __future__ import annotations

import ctypes as C
from typing import List

import torch

from .. import _lib


class ImitationLossOp:
    """Static buffers + the fused loss / gradient kernel for minibatches of a fixed size (modelled on ppo_ops.PpoLossOp).

    `bind(demos)` points the kernel at the demonstration arrays (cand [M,k,n_heads] int64, cand_w [M,k], sample_w [M], returns [M]);
    sample b of a minibatch then reads row `self.rows[b]` of them (GnbvImitationLoss.rows).  `stats` [max_rows + 1, 8] receives one
    row per call at `stats_row`; `flags` is sticky (bit 0: a candidate index out of range, bit 1: a negative or non-finite weight)."""

    def __init__(self, batch: int, head_dims: List[int], k: int, device, max_rows: int, label_smoothing: float = 0.0,
                 ent_coef: float = 0.0, vf_coef: float = 0.0):
        self.lib = _lib.load()
        self.batch, self.head_dims, self.k = int(batch), [int(d) for d in head_dims], int(k)
        n_logits, nh = sum(self.head_dims), len(self.head_dims)
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=device)  # noqa: E731
        self.rows = z(batch, dt=torch.int64)
        self.d_logits, self.d_values = z(batch, n_logits), z(batch)
        self.stats = z(max_rows + 1, 8)
        self.max_rows = int(max_rows)
        self.stats_row = z(1, dt=torch.int64)
        self.flags = z(1, dt=torch.int32)
        self.scratch = z(8 * batch + 64)  # per-sample terms + the completion counter (zero-initialised once)
        a = _lib.GnbvImitationLoss()
        a.batch, a.n_logits, a.n_heads, a.k = self.batch, n_logits, nh, self.k
        for i, d in enumerate(self.head_dims):
            a.head_dims[i] = d
        a.label_smoothing, a.ent_coef, a.vf_coef = float(label_smoothing), float(ent_coef), float(vf_coef)
        a.cand, a.cand_w, a.sample_w, a.returns, a.rows = None, None, None, None, None
        a.d_logits, a.d_values = self.d_logits.data_ptr(), self.d_values.data_ptr()
        a.stats, a.stats_row, a.flags = self.stats.data_ptr(), self.stats_row.data_ptr(), self.flags.data_ptr()
        a.scratch = self.scratch.data_ptr()
        self.args = a
        self.device = device
        self._bound = None

    def bind(self, demos):
        """Fused gather: the kernel reads cand / cand_w / sample_w / returns of rows `self.rows` straight out of `demos` (any object
        with those four tensors; cand_w, sample_w and returns may be None)."""
        a = self.args
        nh = len(self.head_dims)
        cand = demos.cand
        _lib.require_cuda(cand)
        if cand.dtype != torch.int64 or cand.dim() != 3 or cand.shape[1] != self.k or cand.shape[2] != nh or not cand.is_contiguous():
            raise _lib.GennbvHipError(f"ImitationLossOp.bind: cand must be contiguous int64 [M, {self.k}, {nh}], got {cand.dtype} {tuple(cand.shape)}")
        m = cand.shape[0]
        for name, shape in (("cand_w", (m, self.k)), ("sample_w", (m,)), ("returns", (m,))):
            t = getattr(demos, name, None)
            if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != cand.device):
                raise _lib.GennbvHipError(f"ImitationLossOp.bind: {name} must be contiguous float32 {shape} on {cand.device}")
        a.cand = cand.data_ptr()
        a.cand_w, a.sample_w = _lib.ptr(getattr(demos, "cand_w", None)), _lib.ptr(getattr(demos, "sample_w", None))
        a.returns = _lib.ptr(getattr(demos, "returns", None))
        a.rows = self.rows.data_ptr()
        self._bound = demos  # (keeps the arrays alive)

    def __call__(self, logits: torch.Tensor, values: torch.Tensor = None):
        if self._bound is None:
            raise _lib.GennbvHipError("ImitationLossOp: bind(demos) first")
        _lib.require_cuda(logits, values)
        assert logits.is_contiguous() and logits.dtype == torch.float32 and tuple(logits.shape) == (self.batch, self.args.n_logits)
        assert values is None or (values.is_contiguous() and values.dtype == torch.float32 and values.numel() == self.batch)
        self.args.logits, self.args.values = logits.data_ptr(), _lib.ptr(values)
        _lib.check(self.lib.gnbv_imitation_loss(C.byref(self.args), _lib.stream_ptr(self.device)), "gnbv_imitation_loss")
        return self.d_logits, self.d_values
