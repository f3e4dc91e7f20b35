"""Stream order of the stream-taking entry points of include/clm.h.

Every other GPU test runs on torch's default stream, which on ROCm is the legacy null stream and
synchronises implicitly with every blocking stream: a launch, memset or copy on the wrong stream, a
host read ahead of the caller's stream, a workspace reused under a running kernel or a misplaced
fork / join event cannot show there. Here every entry point runs on a torch.cuda.Stream() (created
non-blocking) under stream_order.run_ordered: the device inputs hold poison until a delay on that
stream has run, get the real data on the stream, and are poisoned again behind the call; the clone of
every output, taken on the stream, equals bit for bit what the same call returns on the default
stream with everything synchronised. The poison is always a legal input (stream_order's docstring
states the rule). State-changing calls (append, import, update, remove) run on a fresh index each,
and the states are compared as test_gpu_index_mutate.py compares them: clm_index_export bytes, size,
and a search.

The delay is a chain of dependent 4096 x 4096 fp32 torch.mm calls, doubled by the `delay` fixture
until device events measure DELAY_TARGET_MS (cap DELAY_CAP_MS). test_control_* runs the same harness
with a consumer that is unordered on purpose (a clone() of the input issued on a second side stream,
or on the default stream, with no event wait) and must see the poison in every one of 20 consecutive
trials: if it does not, the delay is too short, or the streams share a hardware queue, and the file
fails instead of passing for the wrong reason.
Measured on an MI355X: 32 matmuls fall short of the target, the chosen chain of 64 measures 58.1 to
58.5 ms, and both controls saw the poison in 20 of 20 trials. Against the library of the commit before
this file (plain hipMemcpy of the ids in clm_index_remove / clm_index_update) all 18 remove / update
cases fail; the clm_index_read cases pass there too.

Entry points of clm.h that take a stream and have no case here: none. Forms of them without a
case: host pointers (the synchronous form; the other suites run it), two streams on one index or
context (clm.h forbids it), the multi-rank paths, clm_gemm's GELU and clm_gemm_ex's PATCH epilogue,
clm_gemm_scores16 mode 2 and clm_layernorm_ex's dual mode (same launch glue as the forms that run).
"""
import contextlib
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import synthetic
from stream_order import Delay, run_ordered, same_bits
from test_gpu_index_mutate import _build, _items, _same_search, _same_state

from clip_lora_match_amd import _capi as C
from clip_lora_match_amd import synthetic as syn
from clip_lora_match_amd.engine import ClipLoraModel
from clip_lora_match_amd.search import GROUP_ROUTE_THRESHOLD, CosineIndex, KeyPlan, key_ranks

pytestmark = pytest.mark.gpu

DELAY_TARGET_MS = 40.0
DELAY_CAP_MS = 300.0
TRIALS = 20


@pytest.fixture(scope="module")
def streams():
    """the side stream every case runs on and the control's second one, made together once: torch
    creates them non-blocking, and the controls prove that this pair and the default stream overlap"""
    return torch.cuda.Stream(), torch.cuda.Stream()


@pytest.fixture(scope="module")
def delay(streams):
    d = Delay()
    d.size(streams[0], DELAY_TARGET_MS, DELAY_CAP_MS)
    print(f"stream-order delay: {d.length} matmuls of 4096^2 fp32 = {d.ms:.1f} ms")
    return d


@pytest.fixture(autouse=True)
def _stop_on_a_device_error():
    """a failed comparison is one test's failure; a device error ends the run (nothing more is
    launched on a device that has faulted)"""
    yield
    try:
        torch.cuda.synchronize()
    except Exception as e:   # noqa: BLE001
        pytest.exit(f"device error after a stream-order case, stopping: {e}", returncode=3)


def _dev(a, dtype=None):
    t = torch.as_tensor(a)
    return t.to(device="cuda", dtype=dtype if dtype is not None else t.dtype).contiguous()


def _other_rows(t):
    """a different finite set of the same shape and dtype"""
    return (t.flip(0).float() * 1.5 + 0.25).to(t.dtype).contiguous()


def _ordered(call, real, poison, delay, streams, make_state=None, what=""):
    exp, got, se, sg = run_ordered(call, real, poison, delay, streams[0], make_state)
    same_bits(exp, got, what or "result")
    return exp, se, sg


# ------------------------------------------------------------------ control --
@pytest.mark.parametrize("consumer", ["side", "default"])
def test_control_unordered_consumer_sees_the_poison(consumer, delay, streams):
    """Pure torch: a clone() on another stream with no event wait must read the poison, every time.
    `side`: a second torch.cuda.Stream(); `default`: the null stream, the one a plain hipMemcpy uses."""
    s, s2 = streams
    real = {"x": torch.arange(1 << 16, dtype=torch.float32, device="cuda")}
    poison = {"x": torch.full((1 << 16,), float("nan"), device="cuda")}
    other = s2 if consumer == "side" else torch.cuda.default_stream()

    def call(_, bufs):
        with torch.cuda.stream(other):
            y = bufs["x"].clone()                      # unordered against the caller's stream
        torch.cuda.current_stream().wait_stream(other)   # the harness may clone y in order
        return y

    for trial in range(TRIALS):
        exp, got, _, _ = run_ordered(call, real, poison, delay, s)
        assert torch.equal(exp, real["x"])
        assert bool(torch.isnan(got).all()), (
            f"trial {trial}: the unordered consumer on the {consumer} stream did not see the poison: the delay "
            f"({delay.length} matmuls, {delay.ms:.1f} ms) is too short or the streams do not overlap")


# ---------------------------------------------------------- index maintenance --
N_IDX = 700      # rows of a fresh index (its capacity starts at 8: every build grows it)
N_NEW = 500      # rows appended / imported on the stream: past the capacity, index_grow runs
OFFSET = 1000
KINDS = ["f16", "f32", "mixed"]
DIMS = [64, 192]


def _fresh(dim, kind, offset=0):
    return lambda: _build(_items(dim, kind, N_IDX), dim, offset)


def _new_rows(dim, kind, n=N_NEW, seed=23):
    t = torch.stack(_items(dim, "f32", n, seed))
    return _dev(t.half() if kind == "f16" else t)


def _same_index(a, b, dim):
    _same_state(a, b)
    _same_search(a, b, torch.stack(_items(dim, "f32", 8, 5)), 10)


def _export_dev(ix, start, n):
    has32 = int(C.lib().clm_index_has_f32(ix._h)) == 1
    r16 = torch.empty((n, ix.dim_p), dtype=torch.float16, device="cuda")
    inv = torch.empty((n,), dtype=torch.float32, device="cuda")
    r32 = torch.empty((n, ix.dim_p), dtype=torch.float32, device="cuda") if has32 else None
    C.check(C.lib().clm_index_export(ix._h, start, n, C.ptr(r16), C.ptr(inv), C.ptr(r32) if has32 else None,
                                     C.stream_of(ix.device)), "clm_index_export")
    return (r16, inv, r32) if has32 else (r16, inv)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dim", DIMS)
def test_append_then_export_device_buffers(dim, kind, delay, streams):
    """append from device rows past the capacity (index_grow), then export to device buffers"""
    rows = _new_rows(dim, kind)

    def call(ix, bufs):
        ix.append(bufs["rows"])
        return _export_dev(ix, N_IDX - 100, N_NEW)

    _, se, sg = _ordered(call, {"rows": rows}, {"rows": _other_rows(rows)}, delay, streams, _fresh(dim, kind))
    assert len(sg) == N_IDX + N_NEW
    _same_index(sg, se, dim)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dim", DIMS)
def test_import_device_buffers(dim, kind, delay, streams):
    src = _build(_items(dim, kind, N_NEW, 29), dim)
    parts = _export_dev(src, 0, N_NEW)
    names = ("r16", "inv", "r32")[:len(parts)]
    real = dict(zip(names, parts))
    poison = {k: _other_rows(v) for k, v in real.items()}

    def call(ix, bufs):
        r32 = bufs.get("r32")
        C.check(C.lib().clm_index_import(ix._h, C.ptr(bufs["r16"]), C.ptr(bufs["inv"]),
                                         C.ptr(r32) if r32 is not None else None, N_NEW, C.stream_of(ix.device)),
                "clm_index_import")
        return len(ix)

    _, se, sg = _ordered(call, real, poison, delay, streams, _fresh(dim, kind))
    _same_index(sg, se, dim)


def _ids(offset, seed=3, m=150):
    rng = np.random.Generator(np.random.PCG64(seed))
    ids = torch.from_numpy(rng.permutation(N_IDX)[:m].astype(np.int64))
    other = (ids + 211) % N_IDX   # other rows of the index, as distinct as ids are
    return _dev(ids + offset), _dev(other + offset)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dim,offset", [(64, 0), (192, 0), (64, OFFSET)])
def test_remove_device_ids_written_on_the_stream(dim, offset, kind, delay, streams):
    ids, other = _ids(offset)

    def call(ix, bufs):
        return ix.remove(bufs["ids"])

    exp, se, sg = _ordered(call, {"ids": ids}, {"ids": other}, delay, streams, _fresh(dim, kind, offset))
    assert exp == ids.numel()
    _same_index(sg, se, dim)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dim,offset", [(64, 0), (192, 0), (64, OFFSET)])
def test_update_device_ids_and_rows_written_on_the_stream(dim, offset, kind, delay, streams):
    ids, other = _ids(offset, seed=4)
    rows = _new_rows(dim, kind, ids.numel(), 31)

    def call(ix, bufs):
        ix.update(bufs["ids"], bufs["rows"])
        return len(ix)

    _, se, sg = _ordered(call, {"ids": ids, "rows": rows}, {"ids": other, "rows": _other_rows(rows)}, delay, streams,
                         _fresh(dim, kind, offset))
    _same_index(sg, se, dim)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dim", DIMS)
def test_read_into_a_device_buffer_the_stream_just_wrote(dim, kind, delay, streams):
    n = 300
    real = {"dst": torch.full((n, dim), 7.0, device="cuda")}
    poison = {"dst": torch.full((n, dim), -3.0, device="cuda")}

    def call(ix, bufs):
        C.check(C.lib().clm_index_read(ix._h, 100, n, C.ptr(bufs["dst"]), C.stream_of(ix.device)), "clm_index_read")
        return bufs["dst"]

    exp, _, _ = _ordered(call, real, poison, delay, streams, _fresh(dim, kind))
    want = torch.stack([r.float() for r in _items(dim, kind, N_IDX)[100:100 + n]])
    assert torch.equal(exp.cpu(), want)


# -------------------------------------------------------------- search routes --
N, NQ, DIM = 3000, 33, 64
N_BIG = 40_000   # the sampled bounded search needs 4 x 8192 rows
SEARCH_ENV = ("CLM_SEARCH_SMALLQ", "CLM_SEARCH_FULL", "CLM_SEARCH_BOUNDED", "CLM_SEARCH_EXACT")


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.pop(k, None) for k in SEARCH_ENV}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k in SEARCH_ENV:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


_shared = {}


def _index(offset=0, n=N, kind="f32"):
    """one resident index per (offset, n, kind) for the calls that leave the rows alone"""
    key = (offset, n, kind)
    if key not in _shared:
        rng = np.random.Generator(np.random.PCG64(41 + n))
        x = torch.from_numpy(rng.standard_normal((n, DIM), dtype=np.float32))
        ix = CosineIndex(DIM, capacity=n)
        ix.append(_dev(x.half() if kind == "f16" else x))
        if offset:
            ix.set_offset(offset)
        _shared[key] = ix
    return _shared[key]


def _q(nq=NQ, seed=7):
    rng = np.random.Generator(np.random.PCG64(seed))
    return _dev(rng.standard_normal((nq, DIM), dtype=np.float32))


def _delta(after, before):
    return {k: after[k] - before[k] for k in after}


# route name -> (environment, the counter that must have served both runs' queries)
SEARCH_ROUTES = {
    "default": ({}, "full_exact"),
    "full": ({"CLM_SEARCH_FULL": "1"}, "full_exact"),
    "bounded_scan": ({"CLM_SEARCH_BOUNDED": "1", "CLM_SEARCH_EXACT": "1"}, "scan_bounded"),
}


@pytest.mark.parametrize("route,offset", [("default", 0), ("default", OFFSET), ("full", 0), ("bounded_scan", 0)])
def test_search_routes(route, offset, delay, streams):
    ix, q = _index(offset), _q()
    env, counter = SEARCH_ROUTES[route]
    before = ix.stats()
    with _env(**env):
        exp, _, _ = _ordered(lambda _, b: ix.search(b["q"], 5), {"q": q}, {"q": _other_rows(q)}, delay, streams)
    d = _delta(ix.stats(), before)
    assert d[counter] == 2 * NQ, d
    assert int(exp[1].min()) >= offset and int(exp[1].max()) < offset + N


def test_search_sampled_bounded_route(delay, streams):
    ix, q = _index(0, N_BIG, "f16"), _q()
    before = ix.stats()
    with _env(CLM_SEARCH_BOUNDED="1"):
        _ordered(lambda _, b: ix.search(b["q"], 5), {"q": q}, {"q": _other_rows(q)}, delay, streams)
    d = _delta(ix.stats(), before)
    assert d["filtered"] == 2 * NQ, d


def test_search_small_batch_route(delay, streams):
    ix, q = _index(), _q(7)
    before = ix.stats()
    with _env(CLM_SEARCH_SMALLQ="1"):
        _ordered(lambda _, b: ix.search(b["q"], 5), {"q": q}, {"q": _other_rows(q)}, delay, streams)
    d = _delta(ix.stats(), before)
    assert d["small_scan"] + d["overflow"] == 2 * 7 and d["small_scan"] > 0, d


def test_search_k_above_1024(delay, streams):
    ix, q = _index(), _q()
    before = ix.stats()
    _ordered(lambda _, b: ix.search(b["q"], 1500), {"q": q}, {"q": _other_rows(q)}, delay, streams)
    assert _delta(ix.stats(), before)["full_exact"] == 2 * NQ


def _words(ix, seed=9):
    rng = np.random.Generator(np.random.PCG64(seed))
    return ix.allow_mask(keep=torch.from_numpy(rng.random(N) < 0.6))


@pytest.mark.parametrize("route,offset", [("default", 0), ("default", OFFSET), ("exact", 0), ("pass", 0), ("gather", 0)])
def test_masked_search_routes(route, offset, delay, streams):
    ix, q = _index(offset), _q()
    words = _words(ix)
    flag = {"default": 0, "exact": C.CLM_MASK_EXACT, "pass": C.CLM_MASK_PASS, "gather": C.CLM_MASK_GATHER}[route]
    before = ix.mask_stats()
    _ordered(lambda _, b: ix.search(b["q"], 5, allow=b["allow"], route=flag), {"q": q, "allow": words},
             {"q": _other_rows(q), "allow": torch.zeros_like(words)}, delay, streams)
    d = _delta(ix.mask_stats(), before)
    assert sum(d.values()) == 2 * NQ, d
    if route == "pass":
        assert d["pass"] > 0 and d["gather"] == 0, d   # a query redone exactly counts as exact
    elif route != "default":
        assert d[route] == 2 * NQ, d


def _key_case(ix):
    rng = np.random.Generator(np.random.PCG64(13))
    values = torch.from_numpy(rng.integers(0, 50, N))
    keys, uniq, cum = key_ranks(_dev(values))
    other = keys.flip(0).contiguous()   # other valid keys: the same ranks on other rows
    lo = _dev(torch.from_numpy(rng.integers(0, 25, NQ)))
    hi = lo + _dev(torch.from_numpy(rng.integers(0, 25, NQ)))
    return keys.contiguous(), other, uniq, cum, lo, hi


@pytest.mark.parametrize("route,offset", [("default", 0), ("default", OFFSET), ("exact", 0), ("pass", 0)])
def test_where_search_routes(route, offset, delay, streams):
    ix, q = _index(offset), _q()
    keys, other, uniq, cum, lo, hi = _key_case(ix)
    flag = {"default": 0, "exact": C.CLM_MASK_EXACT, "pass": C.CLM_MASK_PASS}[route]

    def call(_, b):
        return ix.search_where(b["q"], 5, KeyPlan(b["keys"], uniq, cum, N), b["lo"], b["hi"], route=flag)

    before = ix.where_stats()
    _ordered(call, {"q": q, "keys": keys, "lo": lo, "hi": hi},
             {"q": _other_rows(q), "keys": other, "lo": (lo + 11) % 25, "hi": (lo + 11) % 25 + 3}, delay, streams)
    d = _delta(ix.where_stats(), before)
    assert sum(d.values()) == 2 * NQ, d
    if route == "pass":
        assert d["pass"] > 0, d
    else:
        assert d["exact"] == 2 * NQ, d


@pytest.mark.parametrize("route,offset", [("list", 0), ("list", OFFSET), ("threshold", 0)])
def test_grouped_search_routes(route, offset, delay, streams):
    ix, q = _index(offset), _q()
    rng = np.random.Generator(np.random.PCG64(17))
    groups = _dev(torch.from_numpy(rng.integers(0, 400, N)))
    flag = GROUP_ROUTE_THRESHOLD if route == "threshold" else 0
    before = ix.group_stats()
    _ordered(lambda _, b: ix.search_grouped(b["q"], 5, b["groups"], route=flag), {"q": q, "groups": groups},
             {"q": _other_rows(q), "groups": groups.flip(0).contiguous()}, delay, streams)
    d = _delta(ix.group_stats(), before)
    assert d[route] == 2 * NQ, d


def _targets(offset):
    rng = np.random.Generator(np.random.PCG64(19))
    t = torch.from_numpy(rng.integers(0, N, NQ))
    return _dev(t + offset), _dev((t + 977) % N + offset)


RANK_ROUTES = {"default": (0, "exact"), "exact": (C.CLM_RANK_EXACT, "exact"), "band": (C.CLM_RANK_BAND, "band")}


@pytest.mark.parametrize("route,offset", [("default", 0), ("default", OFFSET), ("exact", 0), ("band", 0)])
def test_rank_routes(route, offset, delay, streams):
    ix, q = _index(offset), _q()
    t, other = _targets(offset)
    flag, counter = RANK_ROUTES[route]
    before = ix.rank_stats()
    _ordered(lambda _, b: ix.rank(b["q"], b["t"], band_cap=flag), {"q": q, "t": t}, {"q": _other_rows(q), "t": other},
             delay, streams)
    d = _delta(ix.rank_stats(), before)
    assert d[counter] == 2 * NQ, d


@pytest.mark.parametrize("route,offset", [("default", 0), ("default", OFFSET), ("exact", 0), ("band", 0)])
def test_count_above_routes(route, offset, delay, streams):
    ix, q = _index(offset), _q()
    t, other = _targets(offset)
    sc = _dev(torch.linspace(-0.2, 0.3, NQ))
    flag, counter = RANK_ROUTES[route]
    before = ix.rank_stats()
    _ordered(lambda _, b: ix.count_above(b["q"], b["s"], b["t"], band_cap=flag), {"q": q, "s": sc, "t": t},
             {"q": _other_rows(q), "s": sc.flip(0).contiguous(), "t": other}, delay, streams)
    d = _delta(ix.rank_stats(), before)
    assert d[counter] == 2 * NQ, d


LSE_ROUTES = {"default": (0, "exact"), "exact": (C.CLM_LSE_EXACT, "exact"), "fast": (C.CLM_LSE_FAST, "fast")}


@pytest.mark.parametrize("route,offset", [("default", 0), ("default", OFFSET), ("exact", 0), ("fast", 0)])
def test_logsumexp_routes(route, offset, delay, streams):
    ix, q = _index(offset), _q()
    flag, counter = LSE_ROUTES[route]
    before = ix.lse_stats()
    _ordered(lambda _, b: ix.logsumexp(b["q"], 1 / 0.07, band_cap=flag), {"q": q}, {"q": _other_rows(q)}, delay,
             streams)
    d = _delta(ix.lse_stats(), before)
    assert d["fast"] + d["exact"] == 2 * NQ, d
    assert d[counter] > 0 and (route == "fast" or d["exact"] == 2 * NQ), d


@pytest.mark.parametrize("offset", [0, OFFSET])
def test_logsumexp64_device_targets(offset, delay, streams):
    ix, q = _index(offset), _q()
    t, other = _targets(offset)
    _ordered(lambda _, b: ix.logsumexp64(b["q"], 1 / 0.07, b["t"]), {"q": q, "t": t},
             {"q": _other_rows(q), "t": other}, delay, streams)


def test_softmax_topk(delay, streams):
    ix, q = _index(), _q()
    _ordered(lambda _, b: ix.softmax_topk(b["q"], 5), {"q": q}, {"q": _other_rows(q)}, delay, streams)


@pytest.mark.parametrize("offset", [0, OFFSET])
def test_softmax_grad_device_lse(offset, delay, streams):
    ix, q = _index(offset), _q()
    scale = 1 / 0.07
    lse, _ = ix.logsumexp(q, scale, head=0)
    rng = np.random.Generator(np.random.PCG64(23))
    row_lse = _dev(torch.from_numpy(rng.uniform(3.0, 5.0, N)))
    before = ix.grad_stats()
    _ordered(lambda _, b: ix.softmax_grad(b["q"], scale, b["lse"], b["row_lse"]),
             {"q": q, "lse": lse, "row_lse": row_lse},
             {"q": _other_rows(q), "lse": lse + 1.0, "row_lse": row_lse.flip(0).contiguous()}, delay, streams)
    assert _delta(ix.grad_stats(), before)["queries"] == 2 * NQ


RANGE_ROUTES = {"default": (0, "exact"), "exact": (C.CLM_RANK_EXACT, "exact"), "band": (C.CLM_RANK_BAND, "fast")}


@pytest.mark.parametrize("route,offset", [("default", 0), ("default", OFFSET), ("exact", 0), ("band", 0)])
def test_search_above_routes_and_read(route, offset, delay, streams):
    """search_above reads the held result back to device buffers (clm_index_search_above_read)"""
    ix, q = _index(offset), _q()
    th = _dev(torch.linspace(0.1, 0.35, NQ))
    flag, counter = RANGE_ROUTES[route]
    before = ix.range_stats()
    exp, _, _ = _ordered(lambda _, b: ix.search_above(b["q"], b["th"], band_cap=flag), {"q": q, "th": th},
                         {"q": _other_rows(q), "th": th.flip(0).contiguous() - 0.05}, delay, streams)
    d = _delta(ix.range_stats(), before)
    assert d[counter] == 2 * NQ, d
    assert int(exp[0][-1]) > NQ   # several rows per query: the ragged result is not trivial


@pytest.mark.parametrize("route,offset", [("default", 0), ("default", OFFSET), ("band", 0)])
def test_search_above_rows_routes(route, offset, delay, streams):
    ix = _index(offset)
    th = _dev(torch.linspace(0.1, 0.35, NQ))
    flag, counter = RANGE_ROUTES[route]
    before = ix.range_stats()
    _ordered(lambda _, b: ix.search_above_rows(offset + 500, NQ, b["th"], band_cap=flag), {"th": th},
             {"th": th.flip(0).contiguous() - 0.05}, delay, streams)
    assert _delta(ix.range_stats(), before)[counter] == 2 * NQ


# -------------------------------------------------------------------- encoder --
N_ENC = 8
_models = {}


def _model(lora_mode, dtype):
    if (lora_mode, dtype) not in _models:
        cfg, sd, lora = synthetic("tiny")
        m = ClipLoraModel(cfg, device="cuda:0", compute_dtype=dtype, lora_mode=lora_mode, max_batch=N_ENC)
        m.load_tensors(sd)
        m.load_tensors(lora)
        m.finalize()
        _models[(lora_mode, dtype)] = m
    return _models[(lora_mode, dtype)]


def _pixels(cfg, layout, seed):
    u8 = torch.from_numpy(syn.images_u8(N_ENC, cfg.image_size, seed))
    if layout == "u8":
        return _dev(u8)
    return _dev(u8.permute(0, 3, 1, 2).float() / 255.0 - 0.5)


def _captions(cfg, seed):
    return _dev(syn.captions(N_ENC, cfg.max_pos, cfg.bos_token_id, cfg.eos_token_id, seed), torch.int32)


MODELS = [("merged", "float16"), ("merged", "bfloat16"), ("unmerged", "float16"), ("unmerged", "bfloat16")]


@pytest.mark.parametrize("layout", ["u8", "f32"])
@pytest.mark.parametrize("lora_mode,dtype", MODELS)
def test_encode_pixels(lora_mode, dtype, layout, delay, streams):
    m = _model(lora_mode, dtype)
    _ordered(lambda _, b: m.encode_pixels(b["pix"]), {"pix": _pixels(m.cfg, layout, 1)},
             {"pix": _pixels(m.cfg, layout, 2)}, delay, streams)


@pytest.mark.parametrize("lora_mode,dtype", MODELS)
def test_encode_ids(lora_mode, dtype, delay, streams):
    m = _model(lora_mode, dtype)
    _ordered(lambda _, b: m.encode_ids(b["ids"]), {"ids": _captions(m.cfg, 3)}, {"ids": _captions(m.cfg, 4)}, delay,
             streams)


@pytest.mark.parametrize("split", [1, 2])
@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("lora_mode,dtype", MODELS)
def test_encode_pair(lora_mode, dtype, graph, split, delay, streams):
    """both towers on the context's own streams, forked from and joined to the caller's; called twice
    on the same buffers with new contents, so that with graph=True the second call is a replay"""
    m = _model(lora_mode, dtype)
    cfg = m.cfg
    real = {"pix": _pixels(cfg, "u8", 1), "ids": _captions(cfg, 3), "pix2": _pixels(cfg, "u8", 5),
            "ids2": _captions(cfg, 6)}
    poison = {"pix": _pixels(cfg, "u8", 2), "ids": _captions(cfg, 4), "pix2": _pixels(cfg, "u8", 7),
              "ids2": _captions(cfg, 8)}

    def call(_, b):
        pix, ids = torch.empty_like(b["pix"]), torch.empty_like(b["ids"])
        oi = torch.empty((N_ENC, cfg.proj_dim), device="cuda")
        ot = torch.empty((N_ENC, cfg.proj_dim), device="cuda")
        res = []
        for p, i in (("pix", "ids"), ("pix2", "ids2")):
            pix.copy_(b[p])
            ids.copy_(b[i])
            m.encode_pair(pix, ids, out_img=oi, out_txt=ot, graph=graph, split=split)
            res += [oi.clone(), ot.clone()]
        return res

    exp, _, _ = _ordered(call, real, poison, delay, streams)
    assert not torch.equal(exp[0], exp[2]) and not torch.equal(exp[1], exp[3])
    # the pair equals the single-tower calls bit for bit (clm.h)
    same_bits(exp[2], m.encode_pixels(real["pix2"]), "pair image rows")
    same_bits(exp[3], m.encode_ids(real["ids2"]), "pair caption rows")


def test_resize_crop_device_buffers(delay, streams):
    S = 32
    rng = np.random.Generator(np.random.PCG64(3))
    shapes = [(45, 70), (33, 32), (120, 51)]
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]
    flat = np.concatenate([a.reshape(-1) for a in imgs])
    sizes = np.array([a.size for a in imgs], np.int64)
    offs = np.zeros(len(imgs), np.int64)
    offs[1:] = np.cumsum(sizes)[:-1]
    hw = np.array(shapes, np.int32).reshape(-1)
    src = _dev(flat)

    def call(_, b):
        out = torch.empty((len(imgs), S, S, 3), dtype=torch.uint8, device="cuda")
        C.check(C.lib().clm_resize_crop(0, C.ptr(b["src"]), offs.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                        hw.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), len(imgs), S, C.ptr(out),
                                        C.stream_of(out.device)), "clm_resize_crop")
        return out

    _ordered(call, {"src": src}, {"src": src.flip(0).contiguous()}, delay, streams)


def test_synth_images_output_consumed_on_the_stream(delay, streams):
    """no inputs: only the output half applies (the clone on the stream sees the finished images)"""
    images = syn.DeviceImages(16, 32, seed=5)
    _ordered(lambda _, b: images.batch(3, 11), {}, {}, delay, streams)


# ---------------------------------------------------------- stand-alone hooks --
# One case each: the kernels have their own tests, the host glue around them is what runs here. Lists
# that a kernel appends to in no fixed order are put into a canonical order before they are compared.
import test_gpu_encoder_ops as EO   # noqa: E402
import test_gpu_fused_attention as FA   # noqa: E402
import test_gpu_gemm_select as GS   # noqa: E402
import test_gpu_gemm_select_keyed as GK   # noqa: E402
import text_plan_ref as P   # noqa: E402
from test_gpu_kernels import _gemm, _ln   # noqa: E402

L_ = C.lib
ST = lambda: C.stream_of(torch.device("cuda:0"))   # noqa: E731


def _randn(seed, *shape, dtype=torch.float32, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype).cuda()


def _pair(seed, *shape, dtype=torch.float32, scale=1.0):
    """(real, poison): two different finite sets"""
    return _randn(seed, *shape, dtype=dtype, scale=scale), _randn(seed + 500, *shape, dtype=dtype, scale=scale)


def _hook(call, named, delay, streams):
    """named: {key: (real, poison)}"""
    return _ordered(call, {k: v[0] for k, v in named.items()}, {k: v[1] for k, v in named.items()}, delay, streams)[0]


def _canon_lists(cnt, cand_s, cand_i, cap):
    """lists appended in no fixed order -> each row sorted by id, unused slots blanked"""
    used = torch.arange(cap, device="cuda")[None, :] < cnt.clamp(max=cap)[:, None].long()
    key = torch.where(used, cand_i, torch.full_like(cand_i, 2 ** 62))
    order = key.argsort(1)
    s = torch.where(used, cand_s, torch.zeros_like(cand_s)).gather(1, order)
    return cnt.clone(), s, key.gather(1, order)


def test_hook_cosine_scores(delay, streams):
    def call(_, b):
        out = torch.empty((33, 300), device="cuda")
        C.check(L_().clm_cosine_scores(0, C.ptr(b["q"]), 33, C.ptr(b["c"]), 300, 100, C.ptr(out), ST()))
        return out
    _hook(call, {"q": _pair(1, 33, 100), "c": _pair(2, 300, 100)}, delay, streams)


def test_hook_topk_merge(delay, streams):
    nq, parts, k_in, k = 33, 3, 8, 10

    def lists(seed):
        g = torch.Generator().manual_seed(seed)
        s = torch.randn((nq, parts, k_in), generator=g).sort(2, descending=True).values
        i = torch.randint(0, 1 << 20, (nq, parts, k_in), generator=g)
        return s.reshape(nq, -1).contiguous().cuda(), i.reshape(nq, -1).contiguous().cuda()
    (s, i), (ps, pi) = lists(3), lists(4)

    def call(_, b):
        os_ = torch.empty((nq, k), device="cuda")
        oi = torch.empty((nq, k), dtype=torch.int64, device="cuda")
        C.check(L_().clm_topk_merge(0, C.ptr(b["s"]), C.ptr(b["i"]), nq, parts, k_in, k, C.ptr(os_), C.ptr(oi), ST()))
        return os_, oi
    _hook(call, {"s": (s, ps), "i": (i, pi)}, delay, streams)


def test_hook_l2_normalize_in_place(delay, streams):
    def call(_, b):
        C.check(L_().clm_l2_normalize(0, C.ptr(b["rows"]), 300, 128, ST()))
        return b["rows"]
    _hook(call, {"rows": _pair(5, 300, 128)}, delay, streams)


def test_hook_fuse_queries(delay, streams):
    def call(_, b):
        out = torch.empty((33, 128), device="cuda")
        C.check(L_().clm_fuse_queries(0, C.ptr(b["a"]), 0.6, C.ptr(b["b"]), 0.4, 33, 128, C.ptr(out), ST()))
        return out
    _hook(call, {"a": _pair(6, 33, 128), "b": _pair(7, 33, 128)}, delay, streams)


@pytest.mark.parametrize("epi", ["STORE", "RESID", "SCORE"])
def test_hook_gemm(epi, delay, streams):
    M, N, K = 333, 200, 128
    named = {"A": _pair(10, M, K, dtype=torch.float16), "W": _pair(11, N, K, dtype=torch.float16, scale=K ** -0.5),
             "bias": _pair(12, N)}
    if epi == "RESID":
        named["out"] = _pair(13, M, N)
    if epi == "SCORE":
        named["rs"], named["cs"] = _pair(14, M), _pair(15, N)

    def call(_, b):
        out = b["out"] if epi == "RESID" else torch.empty((M, N), dtype=torch.float32 if epi == "SCORE" else torch.float16,
                                                          device="cuda")
        _gemm("float16", getattr(C, f"CLM_EPI_{epi}"), -1, b["A"], b["W"], out, None if epi == "SCORE" else b["bias"],
              b.get("rs"), b.get("cs"))
        return out
    _hook(call, named, delay, streams)


def test_hook_gemm_ex_splitk_resid_workspace(delay, streams):
    M, N, K, slices = 129, 200, 768, 4
    named = {"A": _pair(20, M, K, dtype=torch.float16), "W": _pair(21, N, K, dtype=torch.float16, scale=K ** -0.5),
             "bias": _pair(22, N), "out": _pair(23, M, N + 8)}

    def call(_, b):
        ws = torch.empty((slices * M * N + 64,), device="cuda")
        C.check(EO._gemm_ex("float16", C.CLM_EPI_RESID, -1, b["A"], b["W"], M, N, K, b["out"], N + 8, b["bias"],
                            slices=slices, ws=ws), "clm_gemm_ex")
        return b["out"]
    _hook(call, named, delay, streams)


def test_hook_gemm_ex_device_row_count(delay, streams):
    M, N, K = 200, 136, 192
    md = (torch.tensor([77, 0], dtype=torch.int32).cuda(), torch.tensor([200, 0], dtype=torch.int32).cuda())
    named = {"A": _pair(24, M, K, dtype=torch.float16), "W": _pair(25, N, K, dtype=torch.float16, scale=K ** -0.5),
             "bias": _pair(26, N), "m_dev": md}

    def call(_, b):
        out = torch.full((M + 3, N + 8), -99.0, device="cuda").half()
        C.check(EO._gemm_ex("float16", C.CLM_EPI_STORE, -1, b["A"], b["W"], M, N, K, out, N + 8, b["bias"],
                            m_dev=b["m_dev"]), "clm_gemm_ex")
        return out
    exp = _hook(call, named, delay, streams)
    assert bool((exp[77:].float() == -99.0).all()) and not bool((exp[:77, :N].float() == -99.0).any())


def _select_case(seed, M=70, N=1000, K=128):
    return {"A": _pair(seed, M, K, dtype=torch.float16, scale=K ** -0.5), "W": _pair(seed + 1, N, K, dtype=torch.float16),
            "rs": tuple(t.abs() + 0.5 for t in _pair(seed + 2, M)), "cs": tuple(t.abs() + 0.5 for t in _pair(seed + 3, N)),
            "theta": _pair(seed + 4, M)}


def test_hook_gemm_scores16(delay, streams):
    M, N, K = 70, 1024, 128
    named = _select_case(30, N=N)
    del named["theta"]

    def call(_, b):
        out = torch.zeros((M, N), dtype=torch.int16, device="cuda")
        C.check(L_().clm_gemm_scores16(0, 1, C.ptr(b["A"]), K, C.ptr(b["W"]), K, M, N, K, C.ptr(b["rs"]), C.ptr(b["cs"]),
                                       C.ptr(out), N, 1, ST()), "clm_gemm_scores16")
        return out
    _hook(call, named, delay, streams)


def test_hook_gemm_select_masked_and_value_bounds(delay, streams):
    named = _select_case(40)
    g = torch.Generator().manual_seed(44)
    mask = GS._mask_words(torch.rand(1000, generator=g) < 0.6)
    named["mask"] = (mask, torch.zeros_like(mask))

    def call(_, b):
        cb = GS._bounds(b["cs"])
        r = GS.Run(GS.MASK, 1, b["A"], b["W"], b["rs"], b["cs"], b["theta"], cbound=cb, mask=b["mask"], base=5)
        return (cb, r.cnt, r.above) + r.dense()
    exp = _hook(call, named, delay, streams)
    assert int(exp[1][:70].sum()) > 0


def test_hook_gemm_select_rank_and_lse(delay, streams):
    named = _select_case(45)

    def call(_, b):
        res = []
        for epi in (GS.RANK, GS.LSE):
            r = GS.Run(epi, 1, b["A"], b["W"], b["rs"], b["cs"], b["theta"], margin=0.05)
            res += [r.cnt, r.above, r.slab, *r.dense()]
        return res
    _hook(call, named, delay, streams)


def test_hook_gemm_select_keyed(delay, streams):
    M, N, K, cap = 70, 1000, 128, 1000
    A, W, rs, cs, theta, keys, klo, khi, _ = GK._case(M, N, K, 50)
    named = {"A": (A, _other_rows(A)), "W": (W, _other_rows(W)), "rs": (rs, rs.flip(0).contiguous()),
             "cs": (cs, cs.flip(0).contiguous()), "theta": (theta, theta.flip(0).contiguous()),
             "keys": (keys, keys.flip(0).contiguous()), "klo": (klo, klo.flip(0).contiguous()),
             "khi": (khi, khi.flip(0).contiguous())}

    def call(_, b):
        res = GK._keyed(1, b["A"], b["W"], b["rs"], b["cs"], b["theta"], b["keys"], b["klo"], b["khi"], cap, None)
        return (res[0],) + GK._canon(res, N, cap)
    exp = _hook(call, named, delay, streams)
    assert int(exp[0].sum()) > 0


def test_hook_gemm_softw_and_transpose16(delay, streams):
    M, N, K = 70, 1000, 128
    named = _select_case(60)
    del named["theta"]
    named["lq"], named["lr"] = _pair(65, M), _pair(66, N)

    def call(_, b):
        out = torch.zeros((M, N), dtype=torch.int16, device="cuda")
        C.check(L_().clm_gemm_softw(0, -1, C.ptr(b["A"]), K, C.ptr(b["W"]), K, M, N, K, C.ptr(b["rs"]), C.ptr(b["cs"]),
                                    C.ptr(b["lq"]), C.ptr(b["lr"]), 4.0, C.ptr(out), N, ST()), "clm_gemm_softw")
        dst = torch.zeros((K, 128), dtype=torch.int16, device="cuda")
        C.check(L_().clm_transpose16(0, C.ptr(b["A"]), K, M, K, C.ptr(b["rs"]), C.ptr(dst), 128, ST()), "clm_transpose16")
        return out, dst
    _hook(call, named, delay, streams)


@pytest.mark.parametrize("method,k", [(0, 5), (1, 40)])
def test_hook_topk_threshold(method, k, delay, streams):
    nq, Cn, lds = 33, 3000, 3008

    def call(_, b):
        th = torch.empty((nq,), device="cuda")
        C.check(L_().clm_topk_threshold(0, C.ptr(b["s"]), lds, nq, Cn, k, 0.01, method, C.ptr(th), ST()))
        return th
    _hook(call, {"s": _pair(70, nq, lds)}, delay, streams)


def test_hook_scan16_and_collect_ge(delay, streams):
    N_, dim, nq, ldq = 1000, 64, 5, 8
    nchunk = (N_ + 255) // 256
    Wv = int(L_().clm_scan16_waves(0, N_, dim))
    ldw = 8 * Wv + 8
    named = {"rows": _pair(80, N_, dim, dtype=torch.float16), "q16": _pair(81, 16, dim, dtype=torch.float16, scale=0.125),
             "inv": tuple(t.abs() + 0.5 for t in _pair(82, N_)), "qinv": tuple(t.abs() + 0.5 for t in _pair(83, 16)),
             "th": _pair(84, ldq)}

    def call(_, b):
        out = torch.full((N_ + 32, ldq), -77.0, device="cuda")
        cmax = torch.full((nq * nchunk + 64,), -77.0, device="cuda")
        wtop = torch.full((nq + 1, ldw), -77.0, device="cuda")
        C.check(L_().clm_scan16(0, C.ptr(b["rows"]), C.ptr(b["inv"]), N_, dim, C.ptr(b["q16"]), C.ptr(b["qinv"]), nq,
                                C.ptr(out), ldq, C.ptr(cmax), C.ptr(wtop), ldw, ST()), "clm_scan16")
        cnt = torch.zeros((ldq,), dtype=torch.int32, device="cuda")
        cs = torch.zeros((ldq, N_), device="cuda")
        ci = torch.zeros((ldq, N_), dtype=torch.int64, device="cuda")
        C.check(L_().clm_collect_ge(0, C.ptr(out), ldq, nq, N_, C.ptr(b["th"]), C.ptr(cnt), N_, C.ptr(cs), C.ptr(ci),
                                    7, ST()), "clm_collect_ge")
        return (out, cmax, wtop) + _canon_lists(cnt, cs, ci, N_)
    exp = _hook(call, named, delay, streams)
    assert int(exp[3][:nq].sum()) > 0


def test_hook_topk_any(delay, streams):
    nq, Cn, lds, k = 5, 5000, 5005, 1500

    def call(_, b):
        os_ = torch.empty((nq, k), device="cuda")
        oi = torch.empty((nq, k), dtype=torch.int64, device="cuda")
        C.check(L_().clm_topk_any(0, C.ptr(b["s"]), lds, None, 0, nq, Cn, k, 100, C.ptr(os_), C.ptr(oi), ST()))
        return os_, oi
    _hook(call, {"s": _pair(90, nq, lds)}, delay, streams)


def test_hook_mask_rows(delay, streams):
    Nm = 20_000
    g = torch.Generator().manual_seed(95)
    words = GS._mask_words(torch.rand(Nm, generator=g) < 0.4)
    nw, nblk = (Nm + 31) // 32, (Nm + 8191) // 8192

    def call(_, b):
        w = torch.zeros((nw + 1,), dtype=torch.int32, device="cuda")
        bcnt = torch.zeros((nblk + 1,), dtype=torch.int32, device="cuda")
        boff = torch.zeros((nblk + 2,), dtype=torch.int64, device="cuda")
        lst = torch.zeros((Nm + 1,), dtype=torch.int32, device="cuda")
        got_p = ctypes.c_int64(-1)
        C.check(L_().clm_mask_rows(0, C.ptr(b["allow"]), Nm, C.ptr(w), C.ptr(bcnt), C.ptr(boff), C.ptr(lst),
                                   ctypes.byref(got_p), ST()), "clm_mask_rows")
        return w, bcnt, boff, lst, got_p.value
    exp = _hook(call, {"allow": (words, torch.zeros_like(words))}, delay, streams)
    assert exp[4] > 0


def test_hook_topk_distinct(delay, streams):
    nq, ld, k = 33, 200, 10
    ix = _index()

    def lists(seed):
        g = torch.Generator().manual_seed(seed)
        s = torch.randn((nq, ld), generator=g).sort(1, descending=True).values
        return s.cuda(), torch.randint(0, 1 << 20, (nq, ld), generator=g).cuda(), torch.randint(0, 15, (nq, ld), generator=g).cuda()
    a, p = lists(96), lists(97)
    _hook(lambda _, b: ix._topk_distinct(b["s"], b["i"], b["g"], k), {"s": (a[0], p[0]), "i": (a[1], p[1]), "g": (a[2], p[2])},
          delay, streams)


def test_hook_attention_and_attention_ex(delay, streams):
    B, T, H = 5, 77, 2

    def call(_, b):
        res = []
        for ex, flags in ((False, 0), (False, 1), (True, C.CLM_ATTN_CAUSAL), (True, 0)):
            out = torch.zeros((B * T, H * 64), dtype=torch.float16, device="cuda")
            fn = L_().clm_attention_ex if ex else L_().clm_attention
            C.check(fn(0, C.CLM_F16, flags, C.ptr(b["qkv"]), C.ptr(out), out.stride(0), B, T, H, ST()), "clm_attention")
            res.append(out)
        return res
    _hook(call, {"qkv": _pair(100, B * T, 3 * H * 64, dtype=torch.float16)}, delay, streams)


def test_hook_layernorm(delay, streams):
    named = {"x": _pair(110, 77, 512), "g": _pair(111, 512), "b": _pair(112, 512)}
    _hook(lambda _, b: _ln("float16", b["x"], b["g"], b["b"]), named, delay, streams)


def _ids_pair(B, L, vocab, eos, seeds=(1, 2)):
    out = []
    for s in seeds:
        g = torch.Generator().manual_seed(120 + s)
        ids = torch.randint(0, eos, (B, L), generator=g, dtype=torch.int32)
        ids[torch.arange(B), torch.randint(0, L, (B,), generator=g)] = eos
        out.append(ids.cuda())
    return tuple(out)


def test_hook_layernorm_ex_text_embedding(delay, streams):
    """mode 1: token + position embedding and LayerNorm, padded and packed (rowmap / m_dev of a text plan)"""
    d, B, Ln, V, eos = 256, 5, 13, 37, 36
    M = B * Ln
    ids, other = _ids_pair(B, Ln, V, eos)
    named = {"ids": (ids, other), "tok": _pair(121, V, d), "pos": _pair(122, Ln, d), "g": _pair(123, d), "b": _pair(124, d)}

    def call(_, b):
        res = []
        plan = [torch.full((n,), -7, dtype=torch.int32, device="cuda") for n in (B, B + 1, M, B, 2)]
        C.check(L_().clm_text_plan(0, C.ptr(b["ids"]), B, Ln, eos, *(C.ptr(t) for t in plan), ST()), "clm_text_plan")
        for packed in (False, True):
            hf = torch.full((M + 3, d + 4), -99.0, device="cuda")
            y = torch.full((M + 3, d + 8), -99.0, device="cuda").half()
            C.check(EO._ln_ex("float16", 1, M, d, b["g"], b["b"], y, ids=b["ids"], tok=b["tok"], pos=b["pos"], L=Ln, hf=hf,
                              m_dev=plan[4] if packed else None, rowmap=plan[2] if packed else None), "clm_layernorm_ex")
            res += [hf, y]
        return res + plan
    _hook(call, named, delay, streams)


def test_hook_text_plan(delay, streams):
    B, Ln = 37, 77
    ids = torch.from_numpy(P.captions("random", B, Ln, 1)[0]).cuda()
    other = torch.from_numpy(P.captions("runs_256", B, Ln, 2)[0]).cuda()

    def call(_, b):
        plan = [torch.full((n,), -7, dtype=torch.int32, device="cuda") for n in (B, B + 1, B * Ln, B, 2)]
        C.check(L_().clm_text_plan(0, C.ptr(b["ids"]), B, Ln, P.EOS, *(C.ptr(t) for t in plan), ST()), "clm_text_plan")
        return plan
    _hook(call, {"ids": (ids, other)}, delay, streams)


def test_hook_gemm_attn_fixed_length(delay, streams):
    B, T, H, K = 5, 77, 3, 128
    X, W, bias = FA._random_problem(torch.float16, B * T, H, K, 130)
    X2, W2, bias2 = FA._random_problem(torch.float16, B * T, H, K, 131)

    def call(_, b):
        out = torch.full((B * T + 8, H * 64 + 64), -99.0, device="cuda").half()
        assert FA._fused("float16", True, b["X"], b["W"], b["bias"], out, B, T, H, K) == C.CLM_OK
        return out
    _hook(call, {"X": (X, X2), "W": (W, W2), "bias": (bias, bias2)}, delay, streams)


def test_hook_gemm_attn_varlen_device_plan(delay, streams):
    """lens / offs / tiles / counts read from device memory; the poison is the valid plan of another
    caption set, and X and out hold (B + 1) L rows: every plan of B captions stays inside, and so would a
    mixture of two plans"""
    B, Ln, H, K = 37, 77, 3, 128
    plan, _ = FA._plan(P.captions("random", B, Ln, 1)[0], P.EOS)
    other, _ = FA._plan(P.captions("runs_256", B, Ln, 2)[0], P.EOS)
    torch.cuda.synchronize()
    X, W, bias = FA._random_problem(torch.float16, (B + 1) * Ln, H, K, 132)
    X2, _, _ = FA._random_problem(torch.float16, (B + 1) * Ln, H, K, 133)
    named = {"X": (X, X2), "lens": (plan[0], other[0]), "offs": (plan[1], other[1]), "tiles": (plan[2], other[2]),
             "counts": (plan[3], other[3])}

    def call(_, b):
        out = torch.full(((B + 1) * Ln + 8, H * 64 + 64), -99.0, device="cuda").half()
        assert FA._fused("float16", True, b["X"], W, bias, out, B, Ln, H, K,
                         (b["lens"], b["offs"], b["tiles"], b["counts"])) == C.CLM_OK
        return out
    exp = _hook(call, named, delay, streams)
    total = int(plan[3][0])
    assert bool((exp[total:].float() == -99.0).all()) and not bool((exp[:total, :H * 64].float() == -99.0).any())


def test_hook_patchify_and_write_cls(delay, streams):
    B, S, p, Cn, Kp, T, d = 3, 32, 16, 3, 768, 5, 300
    g = torch.Generator().manual_seed(140)
    pix = (torch.randint(0, 256, (B, S, S, Cn), generator=g, dtype=torch.uint8).cuda(),
           torch.randint(0, 256, (B, S, S, Cn), generator=g, dtype=torch.uint8).cuda())
    named = {"pix": pix, "lut": _pair(141, Cn, 256), "cls": _pair(142, d), "pos": _pair(143, T, d)}

    def call(_, b):
        G = S // p
        Pm = torch.full((B * G * G + 3, Kp), -99.0, device="cuda").half()
        C.check(EO._patchify("float16", b["pix"], C.CLM_PIX_U8_HWC, B, S, p, Cn, b["lut"], Pm, Kp), "clm_patchify")
        h = torch.full((B * T + 2, d + 4), -99.0, device="cuda")
        C.check(L_().clm_write_cls(0, C.ptr(h), d + 4, B, T, d, C.ptr(b["cls"]), C.ptr(b["pos"]), ST()), "clm_write_cls")
        return Pm, h
    _hook(call, named, delay, streams)


def test_hook_gather_pooled_and_pool_project(delay, streams):
    B, T, d, D, eos = 6, 77, 256, 64, 36
    ids, other = _ids_pair(B, T, 37, eos, seeds=(3, 4))
    g = torch.Generator().manual_seed(150)
    O = torch.randint(-30000, 30000, (B * T, d + 8), generator=g, dtype=torch.int16).cuda()
    named = {"h": _pair(151, B * T, d + 4), "O": (O, O.flip(0).contiguous()), "ids": (ids, other),
             "gam": _pair(152, d), "bet": _pair(153, d), "projT": _pair(154, d, D, scale=d ** -0.5)}

    def call(_, b):
        h, Ob = b["h"], b["O"]
        hc = torch.full((B + 2, d), -99.0, device="cuda")
        Oc = torch.full((B + 2, d + 16), -99, dtype=torch.int16, device="cuda")
        C.check(L_().clm_gather_pooled(0, C.ptr(h), h.stride(0), C.ptr(Ob), Ob.stride(0), B, T, d, C.ptr(b["ids"]), eos,
                                       C.ptr(hc), C.ptr(Oc), Oc.stride(0), None, ST()), "clm_gather_pooled")
        tmp = torch.full((B + 2, D), -99.0, device="cuda")
        out = torch.full((B + 2, D), -99.0, device="cuda")
        C.check(EO._pool_project(h, B, T, d, b["ids"], eos, b["gam"], b["bet"], b["projT"], D, tmp, out, 1, None),
                "clm_pool_project")
        return hc, Oc, out
    _hook(call, named, delay, streams)
