"""Kernel-level tests of the small-batch search's streaming pass (k_search.hip scan16_kernel and
collect_ge_kernel) through the clm_scan16 / clm_collect_ge hooks, against plain fp64 / numpy
references of the same operations.

The search tests reach these kernels only behind the exact fp64 re-score, where a wrong fp16-pass
score shows only once a true neighbour drops out of the candidate list. Here every score, chunk
maximum and per-wave top-8 entry is checked, at every row width (one template instantiation each),
every score-matrix stride (three store widths), ragged ends, several chunks per wave, and with
sentinels around everything the kernel may not touch.

Inputs are asymmetric -- rows ~ N(0, 1), queries ~ N(0, 1 / dim), and inverse "norms" that are
independent uniform values in [0.5, 1.5] -- so a swapped row, query or norm shows. The score bar
is the one test_gemm_epilogues_vs_torch sets for the same acc * rscale * cscale arithmetic
(EPI_SCORE): |out - ref| <= 1e-4 max|ref| + 1e-6; a misplaced 16-byte piece is wrong by O(1).
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from clip_lora_match_amd import _capi as C

pytestmark = pytest.mark.gpu
SENT = -7777.0    # no score, maximum or -inf pad equals it
CHUNK = 256


def _make(N, dim, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    rows = torch.randn((N, dim), generator=g, device="cuda").half()
    q16 = (torch.randn((16, dim), generator=g, device="cuda") / dim ** 0.5).half()
    inv = torch.rand(N, generator=g, device="cuda") + 0.5
    qinv = torch.rand(16, generator=g, device="cuda") + 0.5
    return SimpleNamespace(N=N, dim=dim, rows=rows, q16=q16, inv=inv, qinv=qinv, ref=_ref(rows, inv, q16, qinv))


def _ref(rows, inv, q16, qinv):
    """[N, 16] fp64: (q . row) * qinv[q] * inv[row]"""
    return (rows.double() @ q16.double().T) * qinv.double()[None, :] * inv.double()[:, None]


@pytest.fixture(scope="module")
def data():
    """data(N, dim): one set of inputs and one reference per (N, dim), shared by every nq (never
    modified); only the latest set is kept, and it is released with the module"""
    held = {}

    def get(N, dim):
        if (N, dim) not in held:
            held.clear()
            held[(N, dim)] = _make(N, dim, 1000 * dim + N % 997)
        return held[(N, dim)]

    yield get
    held.clear()


def _scan(d, nq):
    N, dim = d.N, d.dim
    ldq = 1
    while ldq < nq:
        ldq *= 2
    nchunk = (N + CHUNK - 1) // CHUNK
    W = int(C.lib().clm_scan16_waves(0, N, dim))
    assert W >= 1
    ldw = 8 * W + 8
    out = torch.full((N + 32, ldq), SENT, device="cuda")
    cmax = torch.full((nq * nchunk + 64,), SENT, device="cuda")
    wtop = torch.full((nq + 1, ldw), SENT, device="cuda")
    C.check(C.lib().clm_scan16(0, C.ptr(d.rows), C.ptr(d.inv), N, dim, C.ptr(d.q16), C.ptr(d.qinv), nq, C.ptr(out),
                               ldq, C.ptr(cmax), C.ptr(wtop), ldw, C.stream_of(out.device)), "clm_scan16")
    torch.cuda.synchronize()
    return out, cmax, wtop, ldq, nchunk, W


def _check(d, nq):
    """a-d of the module's contract for one launch"""
    N = d.N
    out, cmax, wtop, ldq, nchunk, W = _scan(d, nq)
    sent = torch.tensor(SENT, device="cuda")
    # a. every score against fp64 (NaN exactly where the reference has it)
    got, ref = out[:N, :nq].double(), d.ref[:, :nq]
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan), "NaN scores differ from the reference's"
    err = float((got - ref)[~nan].abs().max())
    bar = 1e-4 * float(ref[~nan].abs().max()) + 1e-6
    assert err <= bar, f"dim {d.dim} nq {nq}: max |out - ref| {err:.3e} > {bar:.3e}"
    # b. chunk maxima = the maximum of the kernel's own scores, NaN ignored, bit for bit
    own = torch.full((nchunk * CHUNK, nq), -float("inf"), device="cuda")
    own[:N] = torch.where(torch.isnan(out[:N, :nq]), own[:N], out[:N, :nq])
    want_cm = own.view(nchunk, CHUNK, nq).amax(1).T.contiguous()
    cm = cmax[: nq * nchunk].view(nq, nchunk)
    assert torch.equal(cm.view(torch.int32), want_cm.view(torch.int32)), "chunk maxima"
    # c. the 8 largest over the waves' lists = the 8 largest chunk maxima, -inf padded
    pad = torch.full((nq, 8), -float("inf"), device="cuda")
    want_top = torch.cat([cm, pad], 1).topk(8, dim=1).values
    assert not bool((wtop[:nq, : 8 * W] == sent).any()), "a wave left its top-8 list unwritten"
    got_top = wtop[:nq, : 8 * W].topk(8, dim=1).values
    assert torch.equal(got_top, want_top), "per-wave top-8 lists"
    # d. nothing else is written
    assert bool((out[N:] == sent).all()), "score rows past N written"
    for g4 in range(ldq // 4):
        if 4 * g4 >= nq:
            assert bool((out[:, 4 * g4: 4 * g4 + 4] == sent).all()), f"score columns {4 * g4}.. written"
    assert bool((cmax[nq * nchunk:] == sent).all()), "cmax tail written"
    assert bool((wtop[nq] == sent).all()), "wtop row nq written"
    assert bool((wtop[:, 8 * W:] == sent).all()), "wtop columns past 8 W written"


@pytest.mark.parametrize("nq", [1, 2, 3, 4, 5, 8, 9, 16])
@pytest.mark.parametrize("dim", list(range(64, 1025, 64)))
def test_scan16_vs_fp64(data, dim, nq):
    """Every row width x every score stride (ldq 1, 2, 4, 8, 16; nq below and at each): N = 805 is
    three full chunks and a ragged one whose last 16-row block holds 5 rows."""
    _check(data(805, dim), nq)


@pytest.mark.parametrize("nq", [1, 3, 16])
@pytest.mark.parametrize("dim", [64, 192, 512, 1024])
def test_scan16_waves_walk_several_chunks(data, dim, nq):
    """More chunks than waves (2 CUs + 57 chunks, about 146 k rows on 256 CUs): waves take two or
    three chunks each, the LDS ring runs across chunk boundaries, the last chunk is ragged."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nchunk = 2 * cus + 57
    _check(data(CHUNK * nchunk - 156, dim), nq)


def test_scan16_nan_and_inf_rows(data):
    """All-zero rows with an infinite inverse norm score NaN (a single one and a whole chunk of
    them), a row with inverse norm 0 scores 0: NaN exactly where the reference has it, chunk maxima
    ignore NaN (-inf for the all-NaN chunk), everything else as usual."""
    base = data(805, 128)
    rows, inv = base.rows.clone(), base.inv.clone()
    zero = torch.cat([torch.tensor([3], device="cuda"), torch.arange(256, 512, device="cuda")])
    rows[zero] = 0
    inv[zero] = float("inf")
    inv[600] = 0.0
    d = SimpleNamespace(N=805, dim=128, rows=rows, q16=base.q16, inv=inv, qinv=base.qinv,
                        ref=_ref(rows, inv, base.q16, base.qinv))
    assert bool(torch.isnan(d.ref[zero]).all()) and int(torch.isnan(d.ref).sum()) == 16 * zero.numel()
    _check(d, 5)
    _, cmax, _, _, nchunk, _ = _scan(d, 5)
    cm = cmax[: 5 * nchunk].view(5, nchunk)
    assert bool((cm[:, 1] == -float("inf")).all()) and bool(torch.isfinite(cm[:, [0, 2, 3]]).all())


@pytest.mark.parametrize("dim,nq,ldo", [(32, 1, 1), (96, 1, 1), (1088, 1, 1), (64, 17, 32), (64, 5, 4), (64, 3, 3)])
def test_scan16_refusals(dim, nq, ldo):
    """row widths outside 64 .. 1024 step 64, more than 16 queries, a stride below nq or not a power
    of two: CLM_E_ARG, nothing launched"""
    N = 300
    rows = torch.zeros((N, 1088), device="cuda", dtype=torch.float16)
    q16 = torch.zeros((32, 1088), device="cuda", dtype=torch.float16)
    inv, qinv = torch.ones(N, device="cuda"), torch.ones(32, device="cuda")
    out = torch.full((N + 32, 32), SENT, device="cuda")
    cmax = torch.full((32 * 2 + 64,), SENT, device="cuda")
    rc = C.lib().clm_scan16(0, C.ptr(rows), C.ptr(inv), N, dim, C.ptr(q16), C.ptr(qinv), nq, C.ptr(out), ldo,
                            C.ptr(cmax), None, 0, C.stream_of(out.device))
    torch.cuda.synchronize()
    assert rc == C.CLM_E_ARG
    assert bool((out == SENT).all()) and bool((cmax == SENT).all())


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.mark.parametrize("ldq,nq", [(1, 1), (2, 2), (4, 4), (4, 3), (8, 8), (8, 5), (16, 16), (16, 9)])
def test_collect_ge_vs_numpy(ldq, nq):
    """Candidate collection against numpy: few distinct score values (many ties at the threshold),
    NaN and both infinities, thresholds +inf / -inf / a rare and a common data value, an odd row
    count (C * ldq % 4 != 0 at ldq 1 and 2), a base past 2^32, lists that fit and lists that
    overflow the capacity."""
    Cn, cap, base = 4099, 64, 5_000_000_000
    rng = np.random.default_rng(100 * ldq + nq)
    vals = np.array([-1.5, -0.25, 0.0, 0.5, 0.5, 2.0, 3.0, np.nan, np.inf, -np.inf], dtype=np.float32)
    prob = np.array([0.2, 0.2, 0.15, 0.15, 0.1, 0.178, 0.006, 0.01, 0.003, 0.003])
    S = rng.choice(vals, size=(Cn, ldq), p=prob / prob.sum()).astype(np.float32)
    Sd = torch.from_numpy(S).cuda()
    pick = np.array([np.inf, -np.inf, 3.0, 0.5], dtype=np.float32)
    seen_fit = seen_over = False
    for rot in range(4):
        th = pick[(np.arange(ldq) + rot) % 4]
        thd = torch.from_numpy(th).cuda()
        cnt = torch.full((ldq + 1,), -5, device="cuda", dtype=torch.int32)
        cnt[:nq] = 0
        cs = torch.full(((ldq + 1) * cap,), SENT, device="cuda")
        ci = torch.full(((ldq + 1) * cap,), -99, device="cuda", dtype=torch.int64)
        C.check(C.lib().clm_collect_ge(0, C.ptr(Sd), ldq, nq, Cn, C.ptr(thd), C.ptr(cnt), cap, C.ptr(cs), C.ptr(ci),
                                       base, C.stream_of(Sd.device)), "clm_collect_ge")
        torch.cuda.synchronize()
        cnt_h, cs_h, ci_h = cnt.cpu().numpy(), cs.cpu().numpy(), ci.cpu().numpy()
        for q in range(nq):
            with np.errstate(invalid="ignore"):
                hit = np.nonzero(S[:, q] >= th[q])[0]          # NaN never counts
            assert cnt_h[q] == hit.size, (q, th[q])
            want = set(zip(_bits(S[hit, q]).tolist(), (base + hit).tolist()))
            n_st = min(hit.size, cap)
            ls, li = cs_h[q * cap: (q + 1) * cap], ci_h[q * cap: (q + 1) * cap]
            got = list(zip(_bits(ls[:n_st]).tolist(), li[:n_st].tolist()))
            assert len(set(got)) == n_st, "duplicate candidates"
            if hit.size <= cap:
                assert set(got) == want
                assert (ls[n_st:] == SENT).all() and (li[n_st:] == -99).all()
                seen_fit = seen_fit or hit.size > 0
            else:
                assert set(got) <= want
                seen_over = True
        # lists of columns >= nq, and the spare list past the last one: untouched
        assert (cs_h[nq * cap:] == SENT).all() and (ci_h[nq * cap:] == -99).all()
        assert (cnt_h[nq:] == -5).all()
    assert seen_fit and seen_over
