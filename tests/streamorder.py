"""A harness that holds a device entry to stream order, with no host synchronisation around the call.

The synchronous GPU tests drain the stream before an entry and again before they look at anything, so none of them can
see a missing wait between the caller's stream and a stream of the handle's own.  run_ordered() queues everything on ONE
fresh non-default torch stream S, which the handle is given (set_stream), behind a gate that keeps S busy while the
entry is called:

  1. every bulk input is filled with poison A, every output with a sentinel; the device is drained (the only drain)
  2. the gate (torch.cuda._sleep) is queued on S with event E_gate behind it; E_gate must not have happened yet
  3. behind the gate the real input B is copied into the same input buffers from pinned host memory
  4. the entry is called; whether it returned while the gate was closed is noted, not asserted (an entry that hands a
     pageable host table to hipMemcpyAsync may wait there)
  5. still on S, every output is copied to a snapshot and every input overwritten with poison C
  6. S is synchronised: the snapshots must be what the witness says B gives
  7. the device is synchronised: the outputs must still equal their snapshots (nothing lands late from a side stream)
     and the guard words around them must be intact

A, B and C are valid inputs of one geometry whose results differ, so work that ran too early (it saw A), too late (it
saw C) or beside the caller's copies gives a wrong answer, never a wrong access.

The control (control_catches_unordered_copy / control_passes_ordered_copy) runs the same steps on a torch-only stand-in
that copies its input to its output on a second torch stream: without wait_stream it must be caught, with
side.wait_stream(S) before and S.wait_stream(side) after it must pass.

What the control does not establish: that each of the LIBRARY's side streams sits on a hardware queue other than S's.
Two streams that share a queue run in order whatever events they wait for, so a missing wait on a side stream that
aliases S's queue stays invisible here.  That every internal stream of the handle is on a queue of its own is supposed,
not measured.

No GPU work happens at import.
"""
from __future__ import annotations

import os
import time

import numpy as np

GUARD = 64                       # guard elements on either side of every output
GATE_MIN_MS, GATE_MAX_MS, GATE_MARGIN = 20.0, 200.0, 10.0
LOG: list[str] = []              # one line per run_ordered call; written by write_log()

_calib = None                    # (kind, units per millisecond, the callable that queues that many units)


class Bulk:
    """A bulk input: one device buffer and three host versions of it (poison A, the real input B, poison C) in pinned
    memory, all of one shape and dtype."""

    def __init__(self, torch, a, b, c):
        arrs = [np.ascontiguousarray(x) for x in (a, b, c)]
        assert arrs[0].shape == arrs[1].shape == arrs[2].shape and arrs[0].dtype == arrs[1].dtype == arrs[2].dtype
        self.host = [torch.from_numpy(x.copy()).pin_memory() for x in arrs]
        self.dev = torch.empty(arrs[0].shape, dtype=self.host[0].dtype, device="cuda")

    def load(self, which: int, non_blocking: bool = True) -> None:
        self.dev.copy_(self.host[which], non_blocking=non_blocking)


class Guarded:
    """An output of `numel` elements in the middle of a buffer whose first and last GUARD elements, and the output
    itself before the call, hold a sentinel."""

    def __init__(self, torch, numel: int, dtype, sentinel):
        self.torch, self.numel, self.sentinel = torch, int(numel), sentinel
        self.buf = torch.empty(self.numel + 2 * GUARD, dtype=dtype, device="cuda")
        self.win = self.buf[GUARD:GUARD + self.numel]
        self.snap = torch.empty_like(self.buf)
        self.fill()

    def fill(self) -> None:
        self.buf.fill_(self.sentinel)
        self.snap.fill_(self.sentinel)

    def guards_intact(self, host) -> bool:
        s = np.asarray(self.sentinel, dtype=host.dtype)
        return bool((host[:GUARD] == s).all() and (host[GUARD + self.numel:] == s).all())


class Report:
    """What one run_ordered() call saw: failures as (step, output, message); early = the entry returned while the gate
    was closed."""

    def __init__(self, name):
        self.name, self.failures, self.early = name, [], None
        self.t_e_ms = self.gate_ms = 0.0

    def assert_clean(self) -> None:
        assert not self.failures, f"{self.name}: " + "; ".join(f"step {s}, {o}: {m}" for s, o, m in self.failures)


def calibrate(torch):
    """(kind, units per millisecond, run) of the gate, measured once per session: torch.cuda._sleep cycles where torch
    has it, else in-place passes over one large tensor; run(units) queues that many on the current stream."""
    global _calib
    if _calib is not None:
        return _calib
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if hasattr(torch.cuda, "_sleep"):
        units, run = 10 ** 6, torch.cuda._sleep
        kind = "_sleep"
    else:
        big = torch.zeros(1 << 26, dtype=torch.int32, device="cuda")
        units, kind = 8, "add_"

        def run(k, big=big):
            for _ in range(int(k)):
                big.add_(1)
    run(units)                                   # (the first launch loads the kernel)
    torch.cuda.synchronize()
    e0.record()
    run(units)
    e1.record()
    torch.cuda.synchronize()
    ms = max(e0.elapsed_time(e1), 1e-3)
    _calib = (kind, units / ms, run)
    LOG.append(f"calibration: {kind}({units}) took {ms:.3f} ms: {units / ms:.0f} units per ms")
    return _calib


def gate_ms_for(t_e_ms: float) -> float:
    """The gate's length: a harness setting, max(20 ms, 10 x T_e), capped at 200 ms."""
    return min(GATE_MAX_MS, max(GATE_MIN_MS, GATE_MARGIN * t_e_ms))


def queue_gate(torch, ms: float) -> None:
    """The gate on the current stream."""
    _, per_ms, run = calibrate(torch)
    run(max(1, int(per_ms * ms)))


def _check(expected, host):
    """None, or what is wrong with a snapshot: expected is an array (exact equality) or a callable that raises
    AssertionError."""
    if callable(expected):
        try:
            expected(host)
        except AssertionError as e:
            return str(e) or "the witness disagrees"
        return None
    want = np.asarray(expected).reshape(-1)
    if want.dtype != host.dtype or want.shape != host.shape:
        return f"shape or dtype {host.dtype}{host.shape}, expected {want.dtype}{want.shape}"
    bad = np.nonzero(want != host)[0]
    if bad.size:
        i = int(bad[0])
        return f"{bad.size} of {host.size} values differ; first at {i}: got {host[i]!r} expected {want[i]!r}"
    return None


def run_ordered(torch, name, entry, inputs, outputs, expected, set_stream, warm=True) -> Report:
    """The seven steps of the module docstring.  entry(S) queues the call(s) under test; inputs: a list of Bulk;
    outputs: {name: Guarded}; expected: {name: array or checking callable} for a subset of the outputs;
    set_stream(raw stream or None) hands S to whatever the entry runs on.  With warm, the entry first runs twice
    synchronously on B: once so that nothing lazy happens under the gate, once to take T_e."""
    rep = Report(name)
    S = torch.cuda.Stream()
    assert S.cuda_stream != 0, "the harness needs a non-default stream"
    set_stream(S.cuda_stream)
    t_e = 0.0
    if warm:
        with torch.cuda.stream(S):
            for k in range(2):
                for b in inputs:
                    b.load(1)
                S.synchronize()
                t0 = time.perf_counter()
                entry(S)
                S.synchronize()
                t_e = (time.perf_counter() - t0) * 1e3
    rep.t_e_ms, rep.gate_ms = t_e, gate_ms_for(t_e)
    calibrate(torch)
    # 1
    for b in inputs:
        b.load(0, non_blocking=False)
    for o in outputs.values():
        o.fill()
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        # 2
        queue_gate(torch, rep.gate_ms)
        e_gate = torch.cuda.Event()
        e_gate.record(S)
        assert not e_gate.query(), f"harness: the gate of {rep.gate_ms:.0f} ms was open before {name} was called"
        # 3
        for b in inputs:
            b.load(1)
        # 4
        entry(S)
        rep.early = not e_gate.query()
        # 5
        for o in outputs.values():
            o.snap.copy_(o.buf, non_blocking=True)
        for b in inputs:
            b.load(2)
        # 6
        S.synchronize()
    snaps = {k: o.snap.cpu().numpy() for k, o in outputs.items()}
    for k, want in expected.items():
        msg = _check(want, snaps[k][GUARD:GUARD + outputs[k].numel])
        if msg:
            rep.failures.append((6, k, msg))
    # 7
    torch.cuda.synchronize()
    for k, o in outputs.items():
        late = o.buf.cpu().numpy()
        if not np.array_equal(late.view(np.uint8), snaps[k].view(np.uint8)):
            rep.failures.append((7, k, "the output changed after the stream's own snapshot of it"))
        if not o.guards_intact(late):
            rep.failures.append((7, k, "guard words overwritten"))
    set_stream(None)
    log_observation(name, rep.t_e_ms, rep.gate_ms, rep.early,
                    "" if not rep.failures else f"; mismatch reported at step {rep.failures[0][0]}")
    return rep


def log_observation(name, t_e_ms: float, gate_ms: float, early: bool, note: str = "") -> None:
    """One line of the log: early is E_gate.query() == False right after the (first gated) call returned."""
    LOG.append(f"{name}: T_e {t_e_ms:.3f} ms, gate {gate_ms:.0f} ms, "
               f"{'returned while the gate was closed' if early else 'returned after the gate had opened'}{note}")


# ---- the control: torch only ---------------------------------------------------------------------------------------

def _control(torch, ordered: bool, side):
    r = np.random.RandomState(77)
    a, b, c = (r.randint(-2 ** 31, 2 ** 31 - 1, size=1 << 16, dtype=np.int64).astype(np.int32) for _ in range(3))
    inp = Bulk(torch, a, b, c)
    out = Guarded(torch, a.size, torch.int32, -1234567)

    def entry(S):
        if ordered:
            side.wait_stream(S)
        with torch.cuda.stream(side):
            out.win.copy_(inp.dev, non_blocking=True)
        if ordered:
            S.wait_stream(side)

    return run_ordered(torch, f"control ({'ordered' if ordered else 'unordered'} copy on a second stream)", entry,
                       [inp], {"out": out}, {"out": b}, lambda raw: None, warm=False)


def control_catches_unordered_copy(torch, tries: int = 4):
    """The stand-in without wait_stream, on up to `tries` side streams from torch's pool (two streams may share a
    hardware queue and then run in order by accident): the reports; at least one must hold a failure."""
    reps = []
    for _ in range(tries):
        reps.append(_control(torch, False, torch.cuda.Stream()))
        if reps[-1].failures:
            break
    return reps


def control_passes_ordered_copy(torch):
    return _control(torch, True, torch.cuda.Stream())


def write_log() -> None:
    """The session's lines to the file FLAKE_STREAM_ORDER_LOG names, if it names one."""
    path = os.environ.get("FLAKE_STREAM_ORDER_LOG")
    if path and LOG:
        with open(path, "w") as f:
            f.write("\n".join(LOG) + "\n")
