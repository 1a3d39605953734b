"""Harness of the stream-order tests (tests/test_stream_order_gpu.py, tests/test_stream_order_cpu.py).

The contract under test (include/gennbv_hip.h): a function whose last parameter is `void *stream` enqueues ALL of its work -- memsets,
copies, every kernel of a chain -- on that stream, does not synchronise the host, and reads its [host] arguments at call time.

Three pieces:
  * `stream_entry_points()`: the functions of the header that take a stream (the census);
  * `RecordingProxy`: wraps the CDLL and records (name, last argument) of every call, so a test sees which stream handle a wrapper passed;
  * `run_protocol()`: the delayed-input protocol.  The side stream is held by a spin kernel; the real inputs `A` reach the input buffers
    only through copies enqueued BEHIND that spin, so a piece of work that lands on any other stream runs at once, on the decoy inputs
    `D` that the buffers still hold, and either has its output overwritten by the fill that follows the copies, or hands a
    decoy-derived intermediate to a later stage.  Both show as a mismatch with the default-stream result.

Nothing here touches the GPU at import.
"""
from __future__ import annotations

import os
import re
import time
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gennbv_hip.h")
DEV = "cuda:0"

FILL_BYTE = 0xA5        # the non-zero byte pattern of outputs and workspaces (fp32 -2.87e-16, int32 -1515870811, u8 165)
SPIN_PROBE_CYCLES = 30_000_000  # the spin timed once for the cycles-per-millisecond calibration (dp_stress_spin_cycles of the project)
DELAY_MULTIPLE = 10     # the delay = this many times the slowest case's host time for (copies + fills + call) on the default stream
MIN_DELAY_MS = 5.0      # ... and never less: a case that enqueues in 20 us still gets a delay a stray kernel finishes in


# ---------------------------------------------------------------------------------------------------------------- the header census
def header_functions(path: str = HEADER) -> Dict[str, List[str]]:
    """name -> parameter list (strings) of every function include/gennbv_hip.h declares."""
    text = open(path).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)
    text = re.sub(r"typedef\s+struct\s+\w*\s*\{.*?\}\s*\w+\s*;", " ", text, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(gnbv_\w+)\s*\(([^()]*)\)\s*;", text):
        params = [" ".join(p.split()) for p in m.group(2).split(",")]
        out[m.group(1)] = [] if params == ["void"] else params
    return out


def stream_entry_points(path: str = HEADER) -> List[str]:
    """The functions whose parameter list ends in `void *stream`, in header order."""
    return [n for n, p in header_functions(path).items() if p and re.fullmatch(r"void\s*\*\s*stream", p[-1])]


# ------------------------------------------------------------------------------------------------------------- the recording proxy
def handle(x) -> int:
    """A stream argument as an integer (None / NULL -> 0)."""
    if x is None:
        return 0
    v = getattr(x, "value", x)
    return 0 if v is None else int(v)


class RecordingProxy:
    """Stands in for the CDLL of gennbv_amd._lib.load(): every function call is appended to `calls` as (name, last argument) and then
    forwarded.  Install with monkeypatch.setattr(_lib, "_lib", proxy) BEFORE an operator object is built (operators cache self.lib)."""

    def __init__(self, lib):
        object.__setattr__(self, "_real", lib)
        object.__setattr__(self, "calls", [])
        object.__setattr__(self, "_streamed", frozenset(stream_entry_points()))

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        calls = self.calls

        def recorded(*args):
            calls.append((name, args[-1] if args else None))
            return fn(*args)
        recorded.__name__ = name
        return recorded

    def clear(self):
        del self.calls[:]

    def streams(self):
        """[(entry point, stream handle as int)] of the recorded calls that take a stream."""
        return [(n, handle(a)) for n, a in self.calls if n in self._streamed]


def install_proxy(monkeypatch):
    from gennbv_amd import _lib
    proxy = RecordingProxy(_lib.load())
    monkeypatch.setattr(_lib, "_lib", proxy)
    return proxy


# -------------------------------------------------------------------------------------------------------------------- the protocol
@dataclass
class Live:
    """One entry-point call with its buffers on the device.
    I: the input (and in/out state) buffers the call reads; A / D: the staged real and decoy contents of each, same shapes, both VALID.
    O: output and workspace buffers, refilled with FILL_BYTE before every call (names in `zero` with zeros: the header demands a clean
       buffer there -- the reason is the value -- and a misdirected clearing memset of it is then undetectable).
    call(stream): enqueue the work on torch stream `stream`; may return {name: tensor} of outputs it allocated itself.
    compare: names (of O, I or the returned dict) whose contents must match between the runs."""
    I: Dict[str, torch.Tensor]
    A: Dict[str, torch.Tensor]
    D: Dict[str, torch.Tensor]
    O: Dict[str, torch.Tensor]
    call: Callable
    compare: List[str]
    zero: Dict[str, str] = field(default_factory=dict)
    exact: bool = True
    inexact_reason: str = ""
    rtol: float = 0.0
    atol: float = 0.0
    host_ms: float = 0.0
    R_A: Optional[dict] = None
    R_D: Optional[dict] = None


def _bytes(t):
    return t.contiguous().view(-1).view(torch.uint8)


def _fill(live: Live):
    for name, t in live.O.items():
        assert t.is_contiguous(), name
        t.view(-1).view(torch.uint8).fill_(0 if name in live.zero else FILL_BYTE)


def _load(live: Live, staged):
    assert set(staged) == set(live.I), (sorted(staged), sorted(live.I))
    for name, t in live.I.items():
        assert staged[name].shape == t.shape and staged[name].dtype == t.dtype, name
        t.copy_(staged[name], non_blocking=True)


def _enqueue(live: Live, staged, stream):
    """copies of the staged inputs, the fill, the call: all on `stream`; returns the compared tensors (not yet snapshotted)."""
    with torch.cuda.stream(stream):
        _load(live, staged)
        _fill(live)
    extra = live.call(stream) or {}
    got = {}
    for name in live.compare:
        got[name] = extra[name] if name in extra else (live.O[name] if name in live.O else live.I[name])
    return got


def _snapshot(got):
    return {k: v.detach().clone() for k, v in got.items()}


def _same(live: Live, a, b) -> bool:
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if live.exact:
        return bool(torch.equal(_bytes(a), _bytes(b)))
    return bool(torch.allclose(a.double(), b.double(), rtol=live.rtol, atol=live.atol, equal_nan=True))


def reference_runs(live: Live):
    """Steps 1 and 2: A then D on the default stream (the D run leaves O and the workspaces as a stray early kernel would find them),
    the host time of the enqueue sequence (after one warm-up on either stream's allocator pool), and the vacuity check."""
    null = torch.cuda.default_stream()
    _enqueue(live, live.A, null)          # warm-up: lazy hipFuncSetAttribute, module load, allocator pools
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = _enqueue(live, live.A, null)
    live.host_ms = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    live.R_A = _snapshot(got)
    got = _enqueue(live, live.D, null)
    torch.cuda.synchronize()
    live.R_D = _snapshot(got)
    problems = []
    for name in live.compare:
        a, d = live.R_A[name], live.R_D[name]
        if torch.equal(_bytes(a), _bytes(d)):
            problems.append(f"vacuous: output {name} is the same for the real and the decoy inputs")
        if name in live.O and name not in live.zero and bool((_bytes(a) == FILL_BYTE).all()):
            problems.append(f"vacuous: output {name} still holds the fill after the call")
    return problems


def run_protocol(live: Live, side, cycles: int) -> List[str]:
    """Steps 3 to 5 on `side`; returns the list of violations (empty = the call kept the contract).  reference_runs() came first."""
    assert live.R_A is not None
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        torch.cuda._sleep(int(cycles))
    got = _enqueue(live, live.A, side)
    held = not side.query()
    side.synchronize()
    torch.cuda.synchronize()
    problems = []
    if not held:
        problems.append("the side stream had drained when the call returned: a hidden host synchronisation, or the delay is too short")
    for name in live.compare:
        if not _same(live, got[name], live.R_A[name]):
            like_d = _same(live, got[name], live.R_D[name])
            problems.append(f"output {name} differs from the default-stream result" + (" and equals the decoy's result" if like_d else ""))
    return problems


# ------------------------------------------------------------------------------------------------------------------- calibration
_cal = {}


def cycles_per_ms() -> float:
    """torch.cuda._sleep cycles per millisecond, timed once with events."""
    if "cpm" not in _cal:
        torch.cuda._sleep(1000)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.cuda._sleep(SPIN_PROBE_CYCLES)
        e1.record()
        torch.cuda.synchronize()
        _cal["cpm"] = SPIN_PROBE_CYCLES / e0.elapsed_time(e1)
    return _cal["cpm"]


def delay_for(host_ms_values) -> dict:
    """The calibration record: the slowest host time, the delay in ms and in spin cycles."""
    slow = max(host_ms_values)
    ms = max(DELAY_MULTIPLE * slow, MIN_DELAY_MS)
    return {"multiple": DELAY_MULTIPLE, "slowest_host_ms": slow, "delay_ms": ms, "cycles_per_ms": cycles_per_ms(),
            "cycles": int(ms * cycles_per_ms())}


_side = {}
SIDE_CANDIDATES = 12    # torch pool streams tried for one that shares no hardware queue with stream 0


def serialised_with_stream0(stream) -> bool:
    """Does work issued on stream 0 AFTER work on `stream` wait for it on this machine?  The runtime multiplexes streams onto a few
    hardware queues (GPU_MAX_HW_QUEUES); two streams on one queue run in submission order, and a stray launch on stream 0, submitted
    after the delayed copies, would then see the real inputs: the protocol could not flag it.  The probe is the protocol itself, on
    the faulty fake entry point."""
    fake = fake_entry_point(True)
    assert reference_runs(fake) == []
    cycles = delay_for([fake.host_ms])["cycles"]
    return not any("differs" in p for p in run_protocol(fake, stream, cycles))


def side_stream():
    """The one side stream of the module: a torch pool stream (non-blocking, so not implicitly ordered with stream 0) that the probe
    above shows to run beside stream 0.  In a fresh process the first candidate does; in a process that has opened many streams the
    first ones offered may share stream 0's hardware queue.  None found: the timing layer cannot be trusted, and everything fails."""
    if "s" not in _side:
        tried = []
        for _ in range(SIDE_CANDIDATES):
            s = torch.cuda.Stream(device=DEV)
            with torch.cuda.stream(s):
                torch.zeros(16, device=DEV).add_(1)
            s.synchronize()
            tried.append(s)  # (kept alive: the pool hands out the next stream, not this one again)
            if not serialised_with_stream0(s):
                _side["s"], _side["skipped"] = s, len(tried) - 1
                break
        else:
            raise AssertionError(f"none of {SIDE_CANDIDATES} torch pool streams runs beside stream 0 on this machine: a launch on the "
                                 "wrong stream cannot be told from a correct one here")
    return _side["s"]


# -------------------------------------------------------------------------------------------------------- the harness's own test
def fake_entry_point(faulty: bool, n: int = 4099) -> Live:
    """A two-stage "entry point" made of torch ops on valid buffers: tmp = 2 x, y = tmp + 1.  The faulty version issues its first stage
    on the default stream, as a library call with a launch on stream 0 would."""
    g = torch.Generator().manual_seed(5)
    a = torch.rand(n, generator=g).to(DEV)
    d = torch.rand(n, generator=g).to(DEV)
    x = torch.empty(n, device=DEV)
    tmp, y = torch.empty(n, device=DEV), torch.empty(n, device=DEV)

    def call(stream):
        with torch.cuda.stream(torch.cuda.default_stream() if faulty else stream):
            torch.mul(x, 2.0, out=tmp)
        with torch.cuda.stream(stream):
            torch.add(tmp, 1.0, out=y)

    return Live(I={"x": x}, A={"x": a}, D={"x": d}, O={"tmp": tmp, "y": y}, call=call, compare=["y"])
