"""Streaming contrastive-loss gradients on the GPU: the EPI_SOFTW epilogue and the transposing copy
alone (clm_gemm_softw, clm_transpose16), CosineIndex.softmax_grad against the two bounds of DESIGN.md,
and evaluate.contrastive_loss_grad / contrastive_loss_tensor on top.

Yardsticks (tests/loss_grad_ref.py, numpy float64):
  certified   the sums of the caller's own rows: per output row ||got - ref|| <= rho * A + tau,
              (rho, tau) = search.softmax_grad_bound(scale, terms), A = the row's weight mass;
  tight       the same sums of the fp16 operands as the passes read them (clm_index_export; queries
              staged through a second index: rows_to_f16 mode 2 either way) with their fp32 inverse
              norms: (rho_t, tau) = softmax_grad_bound(scale, terms, dim=dim).
Both are asserted per row; the largest measured ratio ||got - ref|| / A per family is printed (DESIGN.md
records the table).
"""
import os

import numpy as np
import pytest
import torch

import loss_grad_ref as R
from clip_lora_match_amd import _capi as C
from clip_lora_match_amd import evaluate as EV
from clip_lora_match_amd.search import CosineIndex, softmax_grad_bound
from test_gpu_rank import _problem

pytestmark = pytest.mark.gpu
LOG2E = 1.4426950408889634
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "contrastive_loss_grad.npz"))


def _dev(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).cuda()


# ---- 1. the epilogue alone -----------------------------------------------------------------------------

def _softw_case(cfg, M, N, K, col, seed):
    """got u16 bits [M + 2, ldo] (sentinel 0x7C01 outside [M, N]) and the float64 weights of the same
    fp16 operands with the relative bound of one element"""
    g = np.random.default_rng(seed)
    A = (g.standard_normal((M, K)) / np.sqrt(K)).astype(np.float16)
    W = (g.standard_normal((N, K)) / np.sqrt(K)).astype(np.float16)
    rs = g.uniform(0.5, 1.5, M).astype(np.float32)
    cs = g.uniform(0.5, 1.5, N).astype(np.float32)
    lq = g.uniform(-2, 2, M).astype(np.float32)
    lr = g.uniform(-2, 2, N + 4).astype(np.float32)
    c = np.float32(4.0)
    ldo = N + (4 if N % 4 == 0 else 3)   # N = 1000: the vector stores; 1 and 255: the ragged path
    out = torch.full((M + 2, ldo), 0x7C01, dtype=torch.int16, device="cuda")
    dA, dW, drs, dcs, dlq, dlr = _dev(A), _dev(W), _dev(rs), _dev(cs), _dev(lq), _dev(lr)
    rc = C.lib().clm_gemm_softw(0, cfg, C.ptr(dA), K, C.ptr(dW), K, M, N, K, C.ptr(drs), C.ptr(dcs), C.ptr(dlq),
                                C.ptr(dlr) if col else None, float(c), C.ptr(out), ldo, None)
    torch.cuda.synchronize()
    a64, w64 = A.astype(np.float64), W.astype(np.float64)
    sc = (a64 @ w64.T) * rs.astype(np.float64)[:, None] * cs.astype(np.float64)[None, :]
    x = sc * float(c)
    want = np.exp2(x - lq.astype(np.float64)[:, None])
    if col:
        want = want + np.exp2(x - lr[:N].astype(np.float64)[None, :])
    # the exponent's error, in bits: fp32 accumulation K 2^-24 sum|a||w| and the two scale products on
    # the score, the fma forming x - l (|x| + |l| + |x - l|) 2^-24; then v_exp_f32 (2^-23), the add
    # (2^-24) and the rounding to fp16 (2^-11)
    mag = (np.abs(a64) @ np.abs(w64).T) * rs.astype(np.float64)[:, None] * cs.astype(np.float64)[None, :]
    ebits = float(c) * (K * 2.0 ** -24 * mag + 3 * 2.0 ** -24 * np.abs(sc)) + 2.0 ** -24 * 2 * (np.abs(x) + 2.0)
    rel = np.expm1(np.log(2.0) * ebits) + 2.0 ** -23 + 2.0 ** -24 + 2.0 ** -11
    return rc, out.cpu().numpy(), want, rel


@pytest.mark.parametrize("col", [False, True])
@pytest.mark.parametrize("cfg", list(C.SOFTW_CONFIGS) + [-1])
def test_softw_epilogue(cfg, col):
    """every config EPI_SOFTW is instantiated on (and the heuristic's choice): N = 1 / 255 take the ragged
    scalar path, N = 1000 the vector stores over several tiles with a partial last one; rows past M and
    columns past N keep the sentinel"""
    worst = 0.0
    for M in (1, 17, 300):
        for N in (1, 255, 1000):
            for K in (64, 192):
                rc, got, want, rel = _softw_case(cfg, M, N, K, col, 7 * M + 3 * N + K)
                assert rc == C.CLM_OK, C.lib().clm_last_error()
                assert (got[M:] == 0x7C01).all() and (got[:, N:] == 0x7C01).all(), (M, N, K)
                val = got[:M, :N].view(np.float16).astype(np.float64)
                ratio = np.abs(val - want) / (rel * want)
                worst = max(worst, float(ratio.max()))
                assert (ratio <= 1.0).all(), (M, N, K, float(ratio.max()))
    print(f"\nsoftw cfg {cfg} col {col}: largest |got - want| / bound {worst:.3f}")


@pytest.mark.parametrize("N", [256, 1000])
def test_softw_vector_path_and_saturation(N):
    """ldo a multiple of 4 takes the vector stores (N = 1000: with a partial last tile); an offset far
    below every score saturates at the largest fp16 instead of storing inf"""
    g = np.random.default_rng(N)
    M, K = 300, 128
    A = (g.standard_normal((M, K)) / np.sqrt(K)).astype(np.float16)
    W = (g.standard_normal((N, K)) / np.sqrt(K)).astype(np.float16)
    lq = g.uniform(-2, 2, M).astype(np.float32)
    lq[5] = -100.0
    lr = g.uniform(-2, 2, N).astype(np.float32)
    dA, dW, dlq, dlr = _dev(A), _dev(W), _dev(lq), _dev(lr)
    outs = []
    for cfg in C.SOFTW_CONFIGS:
        out = torch.full((M + 2, N + 8), 0x7C01, dtype=torch.int16, device="cuda")
        C.check(C.lib().clm_gemm_softw(0, cfg, C.ptr(dA), K, C.ptr(dW), K, M, N, K, None, None, C.ptr(dlq), C.ptr(dlr),
                                       4.0, C.ptr(out), N + 8, None), "clm_gemm_softw")
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert (got[M:] == 0x7C01).all() and (got[:, N:] == 0x7C01).all()
        val = got[:M, :N].view(np.float16).astype(np.float64)
        x = 4.0 * (A.astype(np.float64) @ W.astype(np.float64).T)
        want = np.exp2(x - lq.astype(np.float64)[:, None]) + np.exp2(x - lr.astype(np.float64)[None, :])
        assert (val[5] == 65504.0).all() and np.isfinite(val).all()
        keep = np.arange(M) != 5
        assert (np.abs(val[keep] - want[keep]) <= (2.0 ** -11 + 2e-5) * want[keep]).all()
        outs.append(got)
    # the ragged path computes the same bits element by element
    out = torch.full((M + 2, N + 3), 0x7C01, dtype=torch.int16, device="cuda")
    C.check(C.lib().clm_gemm_softw(0, 1, C.ptr(dA), K, C.ptr(dW), K, M, N, K, None, None, C.ptr(dlq), C.ptr(dlr), 4.0,
                                   C.ptr(out), N + 3, None), "clm_gemm_softw")
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy()[:M, :N], outs[1][:M, :N])
    assert np.array_equal(outs[0][:M, :N], outs[1][:M, :N])


def test_softw_refuses_other_configs_and_bad_arguments():
    A = torch.zeros((16, 64), dtype=torch.float16, device="cuda")
    lq = torch.zeros(16, dtype=torch.float32, device="cuda")
    out = torch.full((16, 16), 0x7C01, dtype=torch.int16, device="cuda")
    call = lambda cfg, **kw: C.lib().clm_gemm_softw(  # noqa: E731
        0, cfg, C.ptr(A), kw.get("lda", 64), C.ptr(A), 64, 16, 16, kw.get("K", 64), None, None,
        C.ptr(lq) if kw.get("lq", True) else None, kw.get("lr"), 1.0, C.ptr(out), kw.get("ldo", 16), None)
    for cfg in (2, 5, 8, 11, 13):
        assert cfg not in C.SOFTW_CONFIGS and call(cfg) == C.CLM_E_HIP
    assert call(C.lib().clm_gemm_num_configs()) == C.CLM_E_ARG
    assert call(1, K=32) == C.CLM_E_ARG and call(1, lda=60) == C.CLM_E_ARG and call(1, ldo=8) == C.CLM_E_ARG
    assert call(1, lq=False) == C.CLM_E_ARG
    assert call(1, lr=ctypes_addr(lq, 4)) == C.CLM_E_ARG   # a misaligned column array
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0x7C01).all()
    assert call(1) == C.CLM_OK


def ctypes_addr(t, off):
    import ctypes
    return ctypes.c_void_p(t.data_ptr() + off)


# ---- 2. the transposing copy alone ---------------------------------------------------------------------

@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("pad", [0, 2])
def test_transpose16(scaled, pad):
    """bit-equal to the numpy statement; the padding columns are zero, what lies past them is untouched.
    pad = 2: leading dimensions that are no multiple of 8 take the element-wise loads and stores"""
    g = np.random.default_rng(11 + pad)
    for rows in (1, 63, 64, 300):
        for cols in (64, 192, 512):
            x = (g.standard_normal((rows, cols)) * np.exp2(g.integers(-12, 4, (rows, 1)))).astype(np.float16)
            s = g.uniform(0.25, 8.0, rows).astype(np.float32)
            lds, rp = cols + pad, (rows + 63) // 64 * 64
            ldd = rp + 8 + pad
            src = torch.zeros((rows, lds), dtype=torch.float16)
            src[:, :cols] = torch.from_numpy(x)
            src = src.cuda()
            dst = torch.full((cols + 1, ldd), 0x7C01, dtype=torch.int16, device="cuda")
            ds = _dev(s)
            C.check(C.lib().clm_transpose16(0, C.ptr(src), lds, rows, cols, C.ptr(ds) if scaled else None, C.ptr(dst), ldd,
                                            None), "clm_transpose16")
            torch.cuda.synchronize()
            got = dst.cpu().numpy()
            want = (x.astype(np.float32) * (s[:, None] if scaled else np.float32(1))).astype(np.float16).T
            assert np.array_equal(got[:cols, :rows], want.view(np.int16)), (rows, cols)
            assert (got[:cols, rows:rp] == 0).all() and (got[:cols, rp:] == 0x7C01).all() and (got[cols:] == 0x7C01).all()
    L = C.lib()
    assert L.clm_transpose16(0, C.ptr(src), 8, 4, 16, None, C.ptr(dst), 64, None) == C.CLM_E_ARG   # lds < cols
    assert L.clm_transpose16(0, C.ptr(src), 16, 65, 16, None, C.ptr(dst), 64, None) == C.CLM_E_ARG  # ldd < 128
    assert L.clm_transpose16(0, None, 16, 4, 16, None, C.ptr(dst), 64, None) == C.CLM_E_ARG
    assert L.clm_transpose16(0, None, 16, 0, 16, None, None, 64, None) == C.CLM_OK


# ---- 3.-5. softmax_grad --------------------------------------------------------------------------------

def _export(ix):
    """(unit rows of the fp16 operands with their fp32 inverse norms, unit rows as the index keeps them), fp64"""
    n = len(ix)
    has32 = int(C.lib().clm_index_has_f32(ix._h))
    r16 = torch.zeros((n, ix.dim_p), dtype=torch.float16)
    inv = torch.zeros((n,), dtype=torch.float32)
    r32 = torch.zeros((n, ix.dim_p), dtype=torch.float32) if has32 else None
    C.check(C.lib().clm_index_export(ix._h, 0, n, C.ptr(r16), C.ptr(inv), C.ptr(r32) if has32 else None,
                                     C.stream_of(ix.device)), "clm_index_export")
    op = r16.numpy().astype(np.float64)[:, :ix.dim] * inv.numpy().astype(np.float64)[:, None]
    kept = (r32 if has32 else r16).numpy().astype(np.float64)[:, :ix.dim]
    return op, R.unit(kept)


def _staged(q):
    """the queries as stage_queries_f16 makes them: appended to an index of their own (rows_to_f16 mode 2)"""
    ix = CosineIndex(q.shape[1], capacity=max(q.shape[0], 1))
    ix.append(q)
    op, kept = _export(ix)
    ix.close()
    return op, kept


def _check_rows(tag, got, ref, mass, rho, tau):
    err = np.linalg.norm(got.astype(np.float64) - ref, axis=1)
    ok = err <= rho * mass + tau
    assert ok.all(), (tag, int((~ok).sum()), float((err / (rho * mass + tau)).max()))
    return float((err / mass).max())


def _run_case(ix, q, scale, sym, worst, tag, **kw):
    """one softmax_grad call checked against both yardsticks; returns (dq, dr)"""
    rop, rtrue = _export(ix)
    qop, qtrue = _staged(q)
    n, nq, dim = rop.shape[0], qop.shape[0], ix.dim
    lse, rlse = R.lse_rows(qtrue, rtrue, scale), (R.lse_rows(rtrue, qtrue, scale) if sym else None)
    dq, dr = ix.softmax_grad(q, scale, lse, row_lse=rlse, wq=1.0, wr=1.0 if sym else 0.0, **kw)
    assert dq.shape == (nq, dim) and dr.shape == (n, dim) and dq.dtype == dr.dtype == torch.float32
    dq, dr = dq.cpu().numpy(), dr.cpu().numpy()
    wr = 1.0 if sym else 0.0
    for name, qu, ru, d in (("certified", qtrue, rtrue, None), ("tight", qop, rop, dim)):
        rq, rr, aq, ar = R.softmax_grad_ref(qu, ru, scale, lse, rlse, 1.0, wr)
        for side, got, ref, mass, terms in (("dq", dq, rq, aq, n), ("dr", dr, rr, ar, nq)):
            rho, tau = softmax_grad_bound(scale, terms, 1.0, wr, dim=d)
            key = (name, side, round(scale, 2), "sym" if sym else "one")
            worst[key] = max(worst.get(key, 0.0), _check_rows((tag, name, side), got, ref, mass, rho, tau))
    return dq, dr


def _print_worst(title, worst):
    print()
    for key in sorted(worst):
        print(f"{title}: {key[0]:9s} {key[1]} scale {key[2]:6.2f} {key[3]}  max ||err|| / A = {worst[key]:.3e}")


@pytest.mark.parametrize("dim", [64, 192, 512])
@pytest.mark.parametrize("N", [1, 255, 3000])
def test_softmax_grad_shapes(N, dim):
    """N = 255: the ragged epilogue and a K granule padded with zeros; 3000: several tiles; nq = 300: a
    split-K accumulation of dr (5 K-steps). One direction and both, at the two scales of the design"""
    worst = {}
    for nq in (1, 17, 300):
        rows, q, _ = _problem(N, dim, nq, 1000 * N + dim + nq)
        ix = CosineIndex(dim, capacity=N)
        ix.append(rows)
        for scale in (1 / 0.07, 100.0):
            for sym in (False, True):
                _run_case(ix, q, scale, sym, worst, (N, dim, nq, scale, sym))
        ix.close()
    _print_worst(f"shapes N {N} dim {dim}", worst)


def test_softmax_grad_small_chunks_and_blocks():
    """chunk_rows = 256 x query_block = 64 over 3000 rows and 300 queries: 12 x 5 passes, the tight bound
    still holds, and the same call gives the same bits"""
    rows, q, _ = _problem(3000, 192, 300, 5)
    ix = CosineIndex(192, capacity=3000)
    ix.append(rows)
    worst = {}
    before = ix.grad_stats()
    dq, dr = _run_case(ix, q, 1 / 0.07, True, worst, "small", chunk_rows=256, query_block=64)
    after = ix.grad_stats()
    assert after["passes"] - before["passes"] == 12 * 5 and after["queries"] - before["queries"] == 300
    dq2, dr2 = _run_case(ix, q, 1 / 0.07, True, worst, "small again", chunk_rows=256, query_block=64)
    assert np.array_equal(dq, dq2) and np.array_equal(dr, dr2)
    # sizes that are no multiple of 64 are rounded up: 200 -> 256, 33 -> 64
    before = ix.grad_stats()
    _run_case(ix, q, 1 / 0.07, False, worst, "rounded", chunk_rows=200, query_block=33)
    assert ix.grad_stats()["passes"] - before["passes"] == 12 * 5
    _print_worst("small chunks", worst)
    ix.close()


def test_softmax_grad_index_variants():
    g = torch.Generator().manual_seed(9)
    n, dim, nq = 1000, 128, 70
    base = torch.randn(n, dim, generator=g)
    q = base[torch.randint(0, n, (nq,), generator=g)] + 0.5 * torch.randn(nq, dim, generator=g)
    worst = {}
    # rows appended as fp16 at scales 0.25 .. 8: stored unnormalised, their scale is in inv alone
    sc = torch.exp2(torch.randint(-2, 4, (n, 1), generator=g).float())
    ix = CosineIndex(dim, capacity=n)
    ix.append((base * sc).half())
    assert not int(C.lib().clm_index_has_f32(ix._h))
    _run_case(ix, q, 1 / 0.07, True, worst, "fp16 rows")
    ix.close()
    # an offset index: dr stays in local row order, nothing else changes; want_rows=False
    ix = CosineIndex(dim, capacity=n)
    ix.append(base)
    dq, dr = _run_case(ix, q, 100.0, True, worst, "no offset")
    ix.set_offset(1000)
    dq2, dr2 = _run_case(ix, q, 100.0, True, worst, "offset")
    assert np.array_equal(dq, dq2) and np.array_equal(dr, dr2)
    _, rtrue = _export(ix)
    lse = R.lse_rows(R.unit(q.numpy()), rtrue, 100.0)
    dq3, none = ix.softmax_grad(q, 100.0, lse, wr=0.0, want_rows=False)
    dq4, _ = ix.softmax_grad(q, 100.0, lse, wr=0.0)
    assert none is None and torch.equal(dq3, dq4)
    # a dim that is no multiple of 64: the padding is stripped
    ix.close()
    ix = CosineIndex(100, capacity=n)
    ix.append(base[:, :100])
    _run_case(ix, q[:, :100].contiguous(), 1 / 0.07, True, worst, "dim 100")
    ix.close()
    _print_worst("variants", worst)


def test_softmax_grad_errors_leave_the_index_usable():
    g = torch.Generator().manual_seed(2)
    rows, q = torch.randn(300, 64, generator=g), torch.randn(9, 64, generator=g)
    ix = CosineIndex(64, capacity=400)
    with pytest.raises(ValueError):
        ix.softmax_grad(q, 10.0, torch.zeros(9), wr=0.0)   # empty
    ix.append(rows)
    lse, _ = ix.logsumexp(q, 10.0)
    rl = torch.zeros(300, dtype=torch.float64)
    ok = ix.softmax_grad(q, 10.0, lse, wr=0.0)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            ix.softmax_grad(q, bad, lse, wr=0.0)
    with pytest.raises(ValueError):
        ix.softmax_grad(q, 10.0, lse, wq=-1.0, wr=0.0)
    with pytest.raises(ValueError):
        ix.softmax_grad(q, 10.0, lse, row_lse=rl, wr=float("nan"))
    with pytest.raises(ValueError):
        ix.softmax_grad(q, 10.0, lse)                        # wr = 1 without row_lse
    with pytest.raises(ValueError):
        ix.softmax_grad(q, 10.0, lse[:8], wr=0.0)
    with pytest.raises(ValueError):
        ix.softmax_grad(q, 10.0, lse, row_lse=rl[:299])
    zq = q.clone()
    zq[4] = 0
    with pytest.raises(ValueError):
        ix.softmax_grad(zq, 10.0, lse, wr=0.0)
    again = ix.softmax_grad(q, 10.0, lse, wr=0.0)
    assert torch.equal(ok[0], again[0]) and torch.equal(ok[1], again[1])
    ix.append(torch.zeros(1, 64))                            # a zero row
    with pytest.raises(ValueError):
        ix.softmax_grad(q, 10.0, lse, wr=0.0)
    ix.remove([300])
    again = ix.softmax_grad(q, 10.0, lse, wr=0.0)
    assert torch.equal(ok[0], again[0]) and torch.equal(ok[1], again[1])
    assert ix.softmax_grad(q[:0], 10.0, lse[:0], wr=0.0)[0].shape == (0, 64)
    zq_, zr_ = ix.softmax_grad(q, 10.0, lse, wq=0.0, wr=0.0)   # no weight at all: zeros, not an error
    assert not zq_.any() and not zr_.any() and zr_.shape == (300, 64)
    s, i = ix.search(q, 3)
    assert i.shape == (9, 3)
    ix.close()


# ---- 7.-9. the loss and its gradient -------------------------------------------------------------------

def _grad_row_bound(rho, tau, mass, x, n, T):
    return (rho * mass + tau) / (2 * n * T * np.linalg.norm(np.asarray(x, dtype=np.float64), axis=1))


def test_contrastive_loss_grad_golden():
    a, b, T = GOLD["a"], GOLD["b"], float(GOLD["T"])
    out = EV.contrastive_loss_grad(a, b, T)
    base = EV.contrastive_loss(a, b, T)
    assert {k: out[k] for k in base} == base                 # the same calls: the same bits
    _, _, aq, ar = R.contrastive_grad_ref(a, b, T)
    n = a.shape[0]
    rho0, tau = softmax_grad_bound(1 / T, n)
    assert out["rho"] >= rho0 and (out["err"] > 0 or out["rho"] == rho0)
    ga, gb = out["grad_image"], out["grad_text"]
    assert ga.dtype == torch.float32 and ga.shape == (n, 64) and ga.is_cuda
    worst = 0.0
    for got, want, mass, x in ((ga, GOLD["grad_a64"], aq, a), (gb, GOLD["grad_b64"], ar, b)):
        err = np.linalg.norm(got.cpu().numpy().astype(np.float64) - want, axis=1)
        # fp32 output: half an ulp of the largest entry per component
        bound = _grad_row_bound(out["rho"], tau, mass, x, n, T) + 2.0 ** -24 * np.abs(want).max() * 8
        assert (err <= bound).all(), float((err / bound).max())
        worst = max(worst, float((err * 2 * n * T * np.linalg.norm(x.astype(np.float64), axis=1) / mass).max()))
    print(f"\ngolden 257 x 64: max ||grad err|| 2 N T |x| / A = {worst:.3e} (rho {out['rho']:.4f})")


def test_contrastive_loss_tensor_autograd():
    g = torch.Generator().manual_seed(4)
    a = torch.randn(300, 64, generator=g)
    b = a + 2.0 * torch.randn(300, 64, generator=g)
    want = EV.contrastive_loss_grad(a, b, 0.07)
    la, lb = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    loss = EV.contrastive_loss_tensor(la, lb)
    assert loss.dim() == 0 and loss.device == la.device and float(loss) == float(torch.tensor(want["loss"]).float())
    loss.backward()
    assert torch.equal(la.grad, want["grad_image"].cpu()) and torch.equal(lb.grad, want["grad_text"].cpu())
    la2, lb2 = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    (2 * EV.contrastive_loss_tensor(la2, lb2)).backward()
    assert torch.equal(la2.grad, 2 * la.grad) and torch.equal(lb2.grad, 2 * lb.grad)
    # inputs on the GPU: the loss and the gradients stay there
    ca, cb = a.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    lc = EV.contrastive_loss_tensor(ca, cb)
    lc.backward()
    assert lc.is_cuda and torch.equal(ca.grad.cpu(), la.grad)


def test_gradient_reaches_a_torch_head():
    """64 -> 64 Linear heads on both sides, 300 pairs: the parameters' gradients against torch's own
    float64 autograd through the full [N, N] logits. Bound: row i of d loss / d embeddings is within
    delta_i = (rho A_i + tau) / (2 N T |e_i|); a head's weight gradient is sum_i g_i x_i^T, so it moves by at
    most sum_i delta_i |x_i| (Frobenius), its bias gradient by sum_i delta_i; fp32 (the gradients' cast,
    the head's own backward over N terms) adds (N + 2) 2^-24 sum_i |g_i| |x_i|. The fp32 forward of the
    head moves a cosine by at most d 2^-22, a weight by the factor exp(that / T): folded into rho."""
    T, n, d = 0.07, 300, 64
    g = torch.Generator().manual_seed(6)
    xa = torch.randn(n, d, generator=g)
    xb = xa + 1.5 * torch.randn(n, d, generator=g)
    ha, hb = torch.nn.Linear(d, d), torch.nn.Linear(d, d)
    EV.contrastive_loss_tensor(ha(xa), hb(xb), T).backward()
    # float64 twin
    ha64, hb64 = torch.nn.Linear(d, d).double(), torch.nn.Linear(d, d).double()
    ha64.load_state_dict({k: v.double() for k, v in ha.state_dict().items()})
    hb64.load_state_dict({k: v.double() for k, v in hb.state_dict().items()})
    ea, eb = ha64(xa.double()), hb64(xb.double())
    ea.retain_grad(), eb.retain_grad()
    ua, ub = ea / ea.norm(dim=1, keepdim=True), eb / eb.norm(dim=1, keepdim=True)
    logits = ua @ ub.T / T
    tgt = torch.arange(n)
    l64 = (torch.nn.functional.cross_entropy(logits, tgt) + torch.nn.functional.cross_entropy(logits.T, tgt)) / 2
    l64.backward()
    _, _, aq, ar = R.contrastive_grad_ref(ea.detach().numpy(), eb.detach().numpy(), T)
    rho, tau = softmax_grad_bound(1 / T, n)
    rho = (1 + rho) * np.exp(d * 2.0 ** -22 / T) - 1
    for head, head64, e, x, mass in ((ha, ha64, ea, xa, aq), (hb, hb64, eb, xb, ar)):
        delta = _grad_row_bound(rho, tau, mass, e.detach().numpy(), n, T)
        xn = x.double().norm(dim=1).numpy()
        gn = e.grad.norm(dim=1).numpy()
        slack = (n + 2) * 2.0 ** -24
        dw = float((head.weight.grad.double() - head64.weight.grad).norm())
        db = float((head.bias.grad.double() - head64.bias.grad).norm())
        bw, bb = float((delta * xn).sum() + slack * (gn * xn).sum()), float(delta.sum() + slack * gn.sum())
        print(f"\nhead: |dW err| {dw:.3e} (bound {bw:.3e})  |db err| {db:.3e} (bound {bb:.3e})")
        assert dw <= bw and db <= bb
        assert dw <= 0.2 * float(head64.weight.grad.norm())   # and it is a gradient, not noise


def test_gradient_step_lowers_the_loss():
    g = torch.Generator().manual_seed(8)
    a = torch.randn(300, 64, generator=g)
    b = a + 2.0 * torch.randn(300, 64, generator=g)
    before = EV.contrastive_loss(a, b, 0.07, head=0)["loss"]
    out = EV.contrastive_loss_grad(a, b, 0.07)
    a2, b2 = a - 0.1 * out["grad_image"].cpu(), b - 0.1 * out["grad_text"].cpu()
    after = EV.contrastive_loss(a2, b2, 0.07, head=0)["loss"]
    print(f"\nloss {before:.6f} -> {after:.6f} after one step of 0.1")
    assert after < before
