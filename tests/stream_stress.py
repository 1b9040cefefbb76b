"""A bounded, deterministic race window for the code that runs on two streams (tests/test_stream_order_gpu.py).

The weight gradients of both engines run on a side stream (qea.ops.SideStream) and meet the main chain only at join(); three staging
sites copy from pinned host memory without waiting.  At test shapes every kernel finishes long before its buffer could be handed out
again, so a missing record_stream, an in-place write under a pending reader or a read before the join gives the right numbers.
Here ONE spin kernel of a known length is put in front of the work under test:

    delayed_side(owner, ms)   the spin goes on owner's side stream.  SideStream.join is wrapped for the duration: the wrapper first
                              lets the MAIN stream run dry (event + host synchronise), then requires that the spin has NOT ended, then
                              joins.  So when the backward reaches its join, every free, reallocation and in-place write of the main
                              chain has been done on the device while every side-stream launch is still pending behind the spin.
    delayed_current(ms)       the spin goes on the current stream; Window.require_open() is the same requirement, called by the test
                              once the host calls under test have returned.

A window that closed early (a delay too short for this host, or a main chain that waited for the side stream before join) is an
assertion failure, never a pass and never a skip; so is a block in which the requirement was never evaluated.  Nothing is repeated
and nothing is provoked: a broken rule shows as wrong numbers read from memory that torch's allocator owns.

The spin is torch.cuda._sleep, whose argument counts ticks of a clock whose rate differs between parts: cycles_per_ms() times one
_sleep(10**7) between two timing events, once per process.  Without torch.cuda._sleep the spin is a chain of fill_ launches on a
256 MB tensor, calibrated the same way (the unit is then one fill).  One spin is at most MAX_MS = 1000 ms and at most one is in
flight: a new window first waits for the end of the previous one.

Two HIP streams may share one hardware queue, and a launch on one then waits for the other's running kernel.  That is correct but
not concurrent, and no window can open on such a pair: delayed_side probes for it (runs_beside_current) and lends the SideStream a
stream that does run beside the main one.  On the MI355X about one side stream in eight of a process was such a one.

D_MS, the delay of the engine cases.  It has to outlast the host's enqueue of one whole backward plus its run time.  Measured on the
MI355X (host time from the spin's enqueue to the return of the wrapper's host synchronisation, under a 1000 ms spin, the engines as
they were before this file existed, inputs [B,1,32,128], B <= 6), the largest of two runs of each case in split_f16 and split_bf16:
MEASURED_MS below.  D_MS = 4 x the largest of these (4 x 25.5 = 102), rounded up to a multiple of 50 ms; the 4 covers a busy shared
host and clock variation (the chain is launch-bound Python).  The cap MAX_MS is far away.  The teeth and staging tests take the same
value: their host work is a few launches and copies."""
import contextlib
import time

import torch

MAX_MS = 1000
MEASURED_MS = {"unet/train": 16.8, "unet/train_bn_groups2": 24.2, "unet/eval_grad": 11.3, "unet/train_switches_off": 9.9,
               "crnn/train": 7.0, "crnn/replica_groups3": 25.5, "crnn/replica_groups3_backward_group2": 4.7,
               "crnn/group_sizes_3_1_2": 5.2, "crnn/bn_eval_grad": 3.7, "crnn/train_switches_off": 4.1}
D_MS = min(MAX_MS, int(-(-4 * max(MEASURED_MS.values()) // 50)) * 50)
assert D_MS == 150

_rate = []                # [units per ms]: _sleep ticks, or fills of _fill_buf
_fill_buf = []
_last_end = []            # the end event of the newest spin


def _spin_units(n):
    if hasattr(torch.cuda, "_sleep"):
        torch.cuda._sleep(int(n))
        return
    if not _fill_buf:
        _fill_buf.append(torch.empty(256 << 20, dtype=torch.uint8, device="cuda"))
    for i in range(int(n)):
        _fill_buf[0].fill_(i & 1)


def cycles_per_ms():
    """Spin units per millisecond on the current device (ticks of torch.cuda._sleep, else fills of a 256 MB tensor): one timed spin per
    process."""
    if not _rate:
        units = 10 ** 7 if hasattr(torch.cuda, "_sleep") else 64
        _spin_units(1)                                           # code object and buffer are there before the timed spin
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _spin_units(units)
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
        assert ms > 0, "the calibration spin took no time"
        _rate.append(units / ms)
    return _rate[0]


class Window:
    """One spin: .start / .delay_end are timing events around it on its stream, .t0 the host time of its enqueue, .chain_ms the host time
    from there to the newest evaluation of the requirement, .checks how often it was evaluated."""

    def __init__(self, ms, stream):
        assert 0 < ms <= MAX_MS, f"one spin is at most {MAX_MS} ms, asked for {ms}"
        rate = cycles_per_ms()
        if _last_end:
            _last_end.pop().synchronize()                        # at most one spin in flight
        self.ms, self.checks, self.chain_ms = ms, 0, None
        self.start, self.delay_end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.t0 = time.perf_counter()
        with torch.cuda.stream(stream):
            self.start.record()
            _spin_units(max(1, round(ms * rate)))
            self.delay_end.record()
        _last_end.append(self.delay_end)

    def require_open(self, what):
        """The spin has not ended: everything the host enqueued since the window opened sits behind it (or ran beside it)."""
        self.chain_ms = (time.perf_counter() - self.t0) * 1e3
        self.checks += 1
        assert not self.delay_end.query(), (
            f"{what}: the {self.ms} ms spin ended before the check, {self.chain_ms:.1f} ms after its enqueue: the delay is too short for "
            "this host, or the work under test waited for the delayed stream; the window proves nothing")

    def close(self):
        self.delay_end.synchronize()
        return self.start.elapsed_time(self.delay_end)           # the spin's real length in ms


PROBE_MS = 10
PROBE_TRIES = 8


def runs_beside_current(stream):
    """Does a kernel on the current stream run while `stream` is busy?  Two HIP streams can share one hardware queue (the runtime
    deals a few queues out to all streams of the process), and then a launch on one waits for the other's running kernel: correct,
    only not concurrent.  Probe: a PROBE_MS spin on `stream`, one tiny kernel on the current stream, a host wait for that kernel;
    beside = the spin is still running then.  A busy host can only turn a yes into a no."""
    rate = cycles_per_ms()
    if _last_end:
        _last_end.pop().synchronize()
    dot = torch.empty(1, device="cuda")
    end, ev = torch.cuda.Event(), torch.cuda.Event()
    with torch.cuda.stream(stream):
        _spin_units(max(1, round(PROBE_MS * rate)))
        end.record()
    dot.fill_(0)
    ev.record()
    ev.synchronize()
    beside = not end.query()
    end.synchronize()
    return beside


@contextlib.contextmanager
def delayed_side(owner, ms):
    """Inside: everything owner's SideStream runs waits behind a spin of `ms`, and join() requires the window to be open once the main
    stream has run dry (see the module's text).  Yields the Window; leaves with both streams idle.
    Where the SideStream's own stream shares a hardware queue with the main stream (runs_beside_current), the main chain would sit
    behind the spin and no window could open: for the duration the SideStream then carries another stream that does run beside the
    main one.  The rules under test are about the order of the two streams' work, whichever stream it is."""
    from qea import ops
    assert ops.overlap_enabled(), "the side stream is switched off: nothing would be delayed"
    side = ops.SideStream.of(owner, torch.device("cuda", torch.cuda.current_device()))
    original, own = ops.SideStream.join, side.side
    for _ in range(PROBE_TRIES):
        if runs_beside_current(side.side):
            break
        side.side = torch.cuda.Stream(own.device)
    else:
        side.side = own
        raise AssertionError(f"none of {PROBE_TRIES} streams runs beside the current one: no window can be opened on this device")
    win = Window(ms, side.side)
    win.own_stream = side.side is own

    def join(self):
        assert self is side, "join() of another SideStream than the delayed one: the delay was put on a stream the code does not use"
        ev = torch.cuda.Event()
        ev.record()                                              # on the current = main stream
        ev.synchronize()
        win.require_open("SideStream.join")
        original(self)

    ops.SideStream.join = join
    try:
        yield win
        assert win.checks, "join() was never called inside delayed_side: the requirement was never evaluated"
    finally:
        ops.SideStream.join = original
        win.close()
        side.side.synchronize()
        side.side = own


@contextlib.contextmanager
def delayed_current(ms):
    """Inside: everything enqueued on the current stream waits behind a spin of `ms`.  Yields the Window; the test calls
    require_open() when the host calls under test have returned.  Leaves with the stream idle."""
    stream = torch.cuda.current_stream()
    win = Window(ms, stream)
    try:
        yield win
        assert win.checks, "require_open() was never called inside delayed_current"
    finally:
        win.close()
        stream.synchronize()
