"""Hostile stream ordering for the stream-taking entry points of include/clm.h (helper of
test_gpu_stream_order.py).

run_ordered() calls an entry point twice: once on torch's default stream with everything
synchronised (the expected result), once on a non-blocking side stream s where

    the device inputs hold POISON until a delay of ordinary torch work on s has run,
    the real data is copied in on s only after that delay,
    the entry point is called (it picks s up through _capi.stream_of),
    every device output is cloned on s,
    and the inputs are poisoned again on s behind the call.

Only work that is ordered on s sees the real data: a launch, memset or copy on another stream, a
host read ahead of s, or a kernel still running when the call's work on s is over reads poison, and
the results differ. Results are compared bit for bit (a NaN must be the same NaN).

THE POISON RULE. Poison must be a LEGAL input of the entry point under test: reading it early has
to give a different answer, never an out-of-range address. So: NaN or other finite values for float
rows, queries, weights and scales; another valid caption for token ids; other in-range row ids for
id lists; all-zero words for masks; other valid keys and ranges; valid lens / offs / tiles / counts
of another caption set for a text plan. Never an id, offset or count that the entry point would
reject or index out of bounds with. An entry point that cannot be given a legal poison gets no case.
"""
import torch

_INT_VIEW = {torch.float64: torch.int64, torch.float32: torch.int32, torch.float16: torch.int16,
             torch.bfloat16: torch.int16}


def bits(t: torch.Tensor) -> torch.Tensor:
    """the bit pattern of a tensor as an integer tensor of the same shape"""
    t = t.contiguous()
    return t.view(_INT_VIEW[t.dtype]) if t.dtype in _INT_VIEW else t


def same_bits(a, b, what="") -> None:
    """nested tuples / lists / dicts of tensors and plain values, compared bit for bit"""
    if isinstance(a, torch.Tensor):
        assert isinstance(b, torch.Tensor), what
        assert a.dtype == b.dtype and a.shape == b.shape, f"{what}: {a.dtype}{tuple(a.shape)} vs {b.dtype}{tuple(b.shape)}"
        x, y = bits(a).cpu(), bits(b).cpu()
        if not torch.equal(x, y):
            bad = torch.nonzero((x != y).reshape(-1)).reshape(-1)
            raise AssertionError(f"{what}: {bad.numel()} of {x.numel()} elements differ from the default-stream "
                                 f"result, first at {bad[:5].tolist()}")
    elif isinstance(a, dict):
        assert isinstance(b, dict) and a.keys() == b.keys(), what
        for k in a:
            same_bits(a[k], b[k], f"{what}[{k!r}]")
    elif isinstance(a, (tuple, list)):
        assert isinstance(b, (tuple, list)) and len(a) == len(b), what
        for n, (x, y) in enumerate(zip(a, b)):
            same_bits(x, y, f"{what}[{n}]")
    else:
        assert a == b, f"{what}: {a!r} vs {b!r}"


def _keep(x):
    """a clone of every device tensor of a result, on the current stream"""
    if isinstance(x, torch.Tensor):
        return x.clone()
    if isinstance(x, dict):
        return {k: _keep(v) for k, v in x.items()}
    if isinstance(x, (tuple, list)):
        return tuple(_keep(v) for v in x)
    return x


class Delay:
    """A chain of `length` dependent n x n fp32 matmuls: ordinary torch work that keeps a stream busy
    for a measured time (no spin kernel)."""

    def __init__(self, n: int = 4096, device="cuda"):
        g = torch.Generator(device=device).manual_seed(1)
        self.a = torch.randn((n, n), generator=g, device=device) / n ** 0.5   # products keep their scale
        self.x = torch.randn((n, n), generator=g, device=device)
        self.y = torch.empty_like(self.x)
        self.length = 1
        self.ms = 0.0

    def run(self) -> None:
        """enqueue the chain on the current stream"""
        x, y = self.x, self.y
        for _ in range(self.length):
            torch.mm(self.a, x, out=y)
            x, y = y, x

    def measure(self, stream) -> float:
        """milliseconds the chain takes on `stream`, by device events (the second of two runs)"""
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            self.run()
            t0.record()
            self.run()
            t1.record()
        stream.synchronize()
        return t0.elapsed_time(t1)

    def size(self, stream, target_ms: float, cap_ms: float) -> None:
        """double the chain until it measures target_ms; AssertionError if that takes more than cap_ms"""
        self.length = 1
        self.ms = self.measure(stream)
        while self.ms < target_ms:
            self.length *= 2
            self.ms = self.measure(stream)
        assert self.ms <= cap_ms, f"the delay chain of {self.length} matmuls takes {self.ms:.0f} ms, cap {cap_ms} ms"


def run_ordered(call, real: dict, poison: dict, delay: Delay, stream, make_state=None):
    """(expected, got, state_expected, state_got). call(state, bufs) -> a result (nested tensors and
    plain values); bufs holds one device tensor per key of real / poison (same shapes and dtypes),
    which call must pass to the entry point as they are (the same memory). make_state() builds the
    fresh state (an index, a model) of one run; None for a stateless entry point. The caller
    compares: same_bits(expected, got), and the states as its subsystem compares them."""
    assert real.keys() == poison.keys()
    for k in real:
        assert real[k].is_cuda and poison[k].is_cuda and real[k].shape == poison[k].shape \
            and real[k].dtype == poison[k].dtype, k
    state_e = make_state() if make_state is not None else None
    bufs = {k: v.clone() for k, v in real.items()}
    torch.cuda.synchronize()
    expected = _keep(call(state_e, bufs))
    torch.cuda.synchronize()

    state_g = make_state() if make_state is not None else None
    bufs = {k: v.clone() for k, v in poison.items()}
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        delay.run()
        for k in bufs:
            bufs[k].copy_(real[k], non_blocking=True)   # the real data exists only after the delay
        got = call(state_g, bufs)
        kept = _keep(got)
        for k in bufs:
            bufs[k].copy_(poison[k], non_blocking=True)   # a kernel still running elsewhere reads this
    stream.synchronize()
    torch.cuda.synchronize()
    return expected, kept, state_e, state_g
