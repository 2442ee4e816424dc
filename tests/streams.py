"""Harness of tests/test_gpu_streams.py: run one op where the caller issues it - a side stream, behind a delay - and return every
output and gradient for a bitwise comparison with the default-stream run.

A case is three callables:

    make(seed, device) -> state     everything the op needs, on the device, built on the CURRENT stream (tensors, models, optimizers)
    staged(state) -> [tensors]      the op's input buffers, in a fixed order (what a trainer's prefetch stream would fill)
    run(state) -> {name: tensor}    the op (and its backward, through torch.autograd.grad with the staged upstream gradients)

Protocol (side_run): `work` = make(decoy seed) and `real` = make(real seed) on the default stream, device synchronised; then, on
`side`: a delay, `work`'s buffers <- `real`'s, the op on `work`.  The decoy is another seed of the same generator: valid values and
valid indices, never NaN or garbage.  A kernel, memset or copy of the op that is issued on any stream but `side` runs during the delay,
on the decoy or on a workspace nothing has written yet, and the result differs from the default-stream run of the real inputs; a
mis-streamed element-wise kernel computes a valid wrong answer, not an out-of-range access.

The delay is a chain of matmuls on `side`, calibrated once per device with events (Delay).  It is at least 20 ms and at least 10 x the
host time the slowest non-blocking op of the list takes to enqueue (HOST_MS collects what every default-stream run took on the host;
test_gpu_streams.py asserts the relation after the list has run), so that every launch of such an op is queued before the copy of the
real inputs can run.  Ops that read back to the host simply block until the delay ends."""
import contextlib
import time

import torch

DELAY_MS = 20.0                 # the floor; Delay.ms is what was measured for the chain actually enqueued
HOST_MS = {}                    # case name -> host milliseconds of its (warm) default-stream run, non-blocking cases only


def cpu_bits(outs):
    """{name: tensor} -> {name: host copy} (call after the producing stream was synchronised)."""
    return {k: v.detach().cpu() for k, v in outs.items() if v is not None}


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return bool(torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8)))


def assert_same(got, want, what):
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for k in want:
        assert same_bits(got[k], want[k]), f"{what}: `{k}` differs from the default-stream run"


def differ(got, want):
    return [k for k in want if not same_bits(got[k], want[k])]


class Delay:
    """A chain of n x n matmuls on the current stream that takes at least `ms` milliseconds, calibrated with events on first use."""
    _by_device = {}

    def __init__(self, device, ms=DELAY_MS, n=2048):
        self.device, self.n = torch.device(device), n
        g = torch.Generator().manual_seed(1)
        self.a = (torch.randn(n, n, generator=g) / n ** 0.5).to(self.device)          # |a @ a| stays O(1): no overflow down the chain
        with torch.cuda.device(self.device):
            self._chain(4)                                                             # warm-up: the BLAS handle and its workspace
            torch.cuda.synchronize(self.device)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); self._chain(16); e1.record()
            torch.cuda.synchronize(self.device)
            self.per_ms = e0.elapsed_time(e1) / 16
        self.set(ms)

    def _chain(self, count):
        # the two scratch matrices are the call's own (allocating launches nothing): two delays may run on two streams at once
        b, c = torch.empty_like(self.a), torch.empty_like(self.a)
        src, dst = self.a, b
        for _ in range(count):
            torch.mm(src, self.a, out=dst)
            src, dst = dst, (c if dst is b else b)

    def set(self, ms):
        """Size the chain for `ms` (with a quarter to spare) and measure what it takes."""
        self.count = max(int(1.25 * ms / self.per_ms) + 1, 2)
        with torch.cuda.device(self.device):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(self.device)
            e0.record(); self._chain(self.count); e1.record()
            torch.cuda.synchronize(self.device)
            self.ms = e0.elapsed_time(e1)
        assert self.ms >= ms, f"the delay chain took {self.ms:.1f} ms, {ms:.1f} wanted"

    def __call__(self):
        self._chain(self.count)

    @classmethod
    def on(cls, device):
        device = torch.device(device)
        d = cls._by_device.get(device)
        if d is None:
            d = cls._by_device[device] = cls(device)
        return d


class Case:
    def __init__(self, name, make, staged, run, seed=1, decoy=2, blocking=False):
        """blocking: the op waits for the device inside the call (a control-block readback, a count): its host time says nothing
        about enqueueing and stays out of HOST_MS."""
        self.name, self.make, self.staged, self.run = name, make, staged, run
        self.seed, self.decoy, self.blocking = seed, decoy, blocking

    def __repr__(self):
        return self.name


_DEFAULT = {}
_between_hook = None            # side_run installs its own for the duration of a run
_between_mark = [None]


def between(*upstream):
    """A case's run() calls this between its forward and its backward, with the staged upstream-gradient buffers.  A forward that
    reads back to the host leaves the stream drained, and a backward enqueued on a drained stream would be a weak test: a launch
    on the wrong stream would find its inputs ready more often than not.  On the side stream this puts the decoy back into the
    upstream buffers, enqueues a second delay and stages the real upstream gradients behind it, so the whole backward is queued
    while the stream is busy.  On the default stream it only notes the time: the host cost of enqueueing the backward."""
    if _between_hook is not None:
        _between_hook(upstream)
    else:
        _between_mark[0] = time.perf_counter()


def _entered(device, enter):
    """enter=False: the current device stays what it is (inputs on another device than the current one)."""
    return torch.cuda.device(device) if enter else contextlib.nullcontext()


def default_run(case: Case, device="cuda:0", seed=None, cache=True, enter=True):
    """The reference: the op on the device's default stream with the real inputs, twice over fresh states, the same bits both times
    (a statement about the baseline alone).  Computed once per (case, device, seed) and shared."""
    seed = case.seed if seed is None else seed
    key = (case.name, str(device), seed, enter)
    if cache and key in _DEFAULT:
        return _DEFAULT[key]
    with _entered(device, enter):
        runs = []
        for i in range(2):
            state = case.make(seed, device)
            torch.cuda.synchronize(device)
            _between_mark[0] = None
            t0 = time.perf_counter()
            outs = case.run(state)
            t1 = time.perf_counter()
            host_ms, mark = (t1 - t0) * 1e3, _between_mark[0]
            torch.cuda.synchronize(device)
            runs.append(cpu_bits(outs))
            del state, outs
        if seed == case.seed:                                # of the second, warm run
            if not case.blocking:
                HOST_MS[case.name] = host_ms
            elif mark is not None:                           # a blocking forward: what follows between() enqueues without waiting
                HOST_MS[case.name + " (backward)"] = (t1 - mark) * 1e3
    bad = differ(runs[1], runs[0])
    assert not bad, f"{case.name}: two default-stream runs of the same inputs differ in {bad}: the baseline is not bitwise repeatable"
    if cache:
        _DEFAULT[key] = runs[0]
    return runs[0]


def stage(work, real, case: Case):
    """work's buffers <- real's, on the current stream."""
    dst, src = case.staged(work), case.staged(real)
    assert len(dst) == len(src) and dst
    with torch.no_grad():
        for d, s in zip(dst, src):
            assert d.shape == s.shape and d.dtype == s.dtype and d.device == s.device, (case.name, d.shape, s.shape)
            d.copy_(s, non_blocking=True)


def side_run(case: Case, side: torch.cuda.Stream, device="cuda:0", after=None, enter=True):
    """Steps 2 and 3 of the protocol -> the results as host tensors.  `after(state)`: extra work inside the stream block (tests of
    the harness itself)."""
    global _between_hook
    delay = Delay.on(device)
    with _entered(device, enter):
        work, real = case.make(case.decoy, device), case.make(case.seed, device)
        decoy = [t.detach().clone() for t in case.staged(work)]

        def hook(upstream):
            dst, src = case.staged(work), case.staged(real)
            late = [i for i, t in enumerate(dst) if any(t is u for u in upstream)]
            assert len(late) == len(upstream), f"{case.name}: between() takes staged buffers"
            with torch.no_grad():
                for i in late:
                    dst[i].copy_(decoy[i], non_blocking=True)
                delay()
                for i in late:
                    dst[i].copy_(src[i], non_blocking=True)
        torch.cuda.synchronize(device)
        with torch.cuda.stream(side):
            delay()
            stage(work, real, case)
            _between_hook = hook
            try:
                outs = case.run(work)
            finally:
                _between_hook = None
            extra = after(work) if after is not None else None
        side.synchronize()
        got = cpu_bits(outs)
        torch.cuda.synchronize(device)           # nothing of this run is in flight when its buffers go back to the allocator
    return (got, extra) if after is not None else got


def check_on_side_stream(case: Case, side, device="cuda:0", enter=True):
    want = default_run(case, device)
    got = side_run(case, side, device, enter=enter)
    assert_same(got, want, f"{case.name} on a side stream of {device}")
    return got
