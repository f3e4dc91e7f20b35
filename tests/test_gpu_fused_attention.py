"""The fused q/k/v projection + attention kernel (k_gemm_attn.hip: gemm_attn, gemm_attn_varlen) through
clm_gemm_attn, on its own:

  * the exact-answer families of tests/attn_families.py (identity weights, so q/k/v equal X exactly)
    at the half-ulp bar, at every T where the tile geometry changes, with a partial last tile, the
    half K-step, a bias, and packed variable-length sequences planned by clm_text_plan;
  * kernels.hpp's contract "bit-identical to gemm(EPI_STORE) + attention()" on random inputs;
  * the refusals; and that a sequence whose rows are not finite changes no other sequence's output."""
import functools

import numpy as np
import pytest
import torch

import attn_families as F
import text_plan_ref as P

from clip_lora_match_amd import _capi as C

pytestmark = pytest.mark.gpu
DT = {"bfloat16": (torch.bfloat16, C.CLM_BF16), "float16": (torch.float16, C.CLM_F16)}
K_ID = 3 * F.D   # the identity weight: K = 3 d = 576


def _p(t):
    return C.ptr(t) if t is not None else None


def _fused(dtype, causal, X, W, bias, out, B, T, H, K, plan=(None,) * 4, ldx=None, ldo=None):
    """clm_gemm_attn -> return code; plan = (lens, offs, tiles, counts) device tensors or Nones"""
    return C.lib().clm_gemm_attn(0, DT[dtype][1], C.CLM_ATTN_CAUSAL if causal else 0, C.ptr(X),
                                 X.stride(0) if ldx is None else ldx, C.ptr(W), W.stride(0), _p(bias), C.ptr(out),
                                 out.stride(0) if ldo is None else ldo, B, T, H, K, *(_p(t) for t in plan),
                                 C.stream_of(X.device))


def _two_kernels(dtype, causal, X, W, bias, out, B, T, H, K):
    """the same through clm_gemm(STORE, N = 3 d) + clm_attention; returns the QKV tensor"""
    qkv = torch.empty((B * T, 3 * H * 64), dtype=X.dtype, device=X.device)
    C.check(C.lib().clm_gemm(0, DT[dtype][1], C.CLM_EPI_STORE, -1, C.ptr(X), X.stride(0), C.ptr(W), W.stride(0), B * T,
                             3 * H * 64, K, C.ptr(qkv), qkv.stride(0), _p(bias), None, None, C.stream_of(X.device)),
            "clm_gemm")
    C.check(C.lib().clm_attention(0, DT[dtype][1], int(causal), C.ptr(qkv), C.ptr(out), out.stride(0), B, T, H,
                                  C.stream_of(X.device)), "clm_attention")
    return qkv


def _plan(ids, eos):
    """clm_text_plan on ids [B, L] -> ((lens, offs, tiles, counts) on the device, rowmap on the device)"""
    B, L = ids.shape
    dev = torch.from_numpy(ids).cuda()
    lens, offs, rowmap, tiles, counts = (torch.full((n,), P.SENTINEL, dtype=torch.int32, device="cuda")
                                         for n in (B, B + 1, B * L, B, 2))
    C.check(C.lib().clm_text_plan(0, C.ptr(dev), B, L, eos, C.ptr(lens), C.ptr(offs), C.ptr(rowmap), C.ptr(tiles),
                                  C.ptr(counts), C.stream_of(dev.device)), "clm_text_plan")
    return (lens, offs, tiles, counts), rowmap


def _identity(td, ld=K_ID):
    w = torch.zeros((K_ID, ld), device="cuda")
    w[:, :K_ID] = torch.eye(K_ID, device="cuda")
    return w.to(td)


def _to_dev(a, td, ld=None):
    """numpy [rows, K_ID] -> device tensor of type td, exactly, zero-padded to ld columns"""
    t = torch.from_numpy(np.array(a, dtype=np.float32))   # a copy: the cached cases are read-only
    if ld is not None and ld != t.shape[1]:
        t = torch.cat([t, torch.zeros((t.shape[0], ld - t.shape[1]))], 1)
    d = t.cuda().to(td)
    assert torch.equal(d.float().cpu(), t)
    return d


def _hold_to_bar(out, rows, ref, dtype, what, seq_of=None):
    """out [rows + PAD_ROWS, LDO]: columns past d and rows past `rows` keep the sentinel, the rest meets
    the half-ulp bar against ref. Returns the largest |out - ref|."""
    got = out.double().cpu().numpy()
    assert (got[:, F.D:] == F.SENTINEL).all(), ("columns past d written", what)
    assert (got[rows:] == F.SENTINEL).all(), ("rows past the last sequence written", what)
    got = got[:rows, :F.D]
    err = np.abs(got - ref)
    bad = F.violations(got, ref, dtype)
    if bad.any():
        r, c = np.argwhere(bad)[0]
        where = seq_of(r) if seq_of else ""
        raise AssertionError(f"{what}: {int(bad.sum())} elements in {int(bad.any(1).sum())} rows off the bar, max |err| "
                             f"{err.max():.3e}; first at row {r} {where} col {c} (head {c // F.HD}): got {got[r, c]}, "
                             f"want {ref[r, c]}")
    return float(err.max())


@functools.lru_cache(maxsize=None)
def _batch_ref(family, T, causal, nb):
    """(case, fp64 reference) of make_batch, computed once for both dtypes"""
    case = F.make_batch(family, T, causal, nb)
    ref, p = F.reference(case.qkv, T, causal, nb=nb)
    assert F.leak(case, p) <= F.LEAK_CAP
    ref.setflags(write=False)
    return case, ref


def _run_family(family, T, causal, dtype, nb, K=K_ID, bias=None):
    td = DT[dtype][0]
    case, ref = _batch_ref(family, T, causal, nb)
    ld = (K + 63) // 64 * 64
    x = case.qkv if bias is None else case.qkv - bias[None, :]
    X, W = _to_dev(x, td, ld), _identity(td, ld)
    bdev = None if bias is None else torch.from_numpy(bias.astype(np.float32)).cuda()
    out = torch.full((nb * T + F.PAD_ROWS, F.LDO), F.SENTINEL, device="cuda").to(td)
    what = (family, T, "causal" if causal else "full", dtype, f"B {nb}", f"K {K}")
    assert _fused(dtype, causal, X, W, bdev, out, nb, T, F.H, K) == C.CLM_OK, what
    return _hold_to_bar(out, nb * T, ref, dtype, what, lambda r: f"(sequence {r // T}, query {r % T})")


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
@pytest.mark.parametrize("T", F.FUSED_T)
def test_fused_families_fixed_length(dtype, T):
    """gemm_attn at every T where G = 256 // T, the key tiles or the causal nkt change, with B = G + 1
    (one sequence in the last tile, its rows clamped to M - 1) and B = 2 G - 1: single and pair without
    a mask, causal_pairs and single with it. Neighbouring sequences are different items, so a sequence
    offset that is one off moves the answers by >= 0.5."""
    errs = {}
    for nb in F.fused_batches(T):
        for family, causal in F.FUSED_FAMILIES:
            errs[(nb, family, causal)] = _run_family(family, T, causal, dtype, nb)
    print(f"gemm_attn {dtype} T {T}: max |out - ref64| {max(errs.values())}")


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
@pytest.mark.parametrize("T", [50, 77])
def test_fused_families_half_k_step(dtype, T):
    """K = 608 (K % 64 == 32): the identity padded with 32 zero columns, rows allocated to 640; the last
    K-step multiplies its first 32 columns only"""
    for family, causal in F.FUSED_FAMILIES:
        _run_family(family, T, causal, dtype, 256 // T + 1, K=K_ID + 32)


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
@pytest.mark.parametrize("T", [33, 77])
def test_fused_families_bias(dtype, T):
    """an integer bias in [-3, 3] per column with X = qkv - bias (still exact): acc + bias is qkv"""
    bias = np.random.default_rng(T).integers(-3, 4, K_ID).astype(np.float64)
    for family, causal in F.FUSED_FAMILIES:
        _run_family(family, T, causal, dtype, 256 // T + 1, bias=bias)


@functools.lru_cache(maxsize=None)
def _item_ref(family, T):
    """per item of the causal case at length T: (qkv [2][T, 3 D], reference [2][T, D])"""
    case = F.make(family, T, True)
    ref, p = F.reference(case.qkv, T, True)
    assert F.leak(case, p) <= F.LEAK_CAP
    return case.qkv.reshape(2, T, 3 * F.D), ref.reshape(2, T, F.D)


def _varlen_lens(pattern, B, L):
    if pattern == "ones":
        return np.ones(B, dtype=np.int64)
    if pattern == "full":
        return np.full(B, L)
    if pattern == "alternating":
        return np.where(np.arange(B) % 2 == 0, L, 1)
    if pattern == "random":
        return np.random.default_rng([B, L]).integers(1, L + 1, B)
    assert pattern == "runs_256"
    return P.runs_256(B, L)


VARLEN_PATTERNS = ("ones", "full", "alternating", "random", "runs_256")


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
@pytest.mark.parametrize("family", ["causal_pairs", "single"])
@pytest.mark.parametrize("B", [3, 37, 300])
@pytest.mark.parametrize("L", [16, 77, 128])
def test_fused_families_varlen(dtype, family, L, B):
    """gemm_attn_varlen on packed sequences planned by clm_text_plan from ids, as the engine chains the
    two: sequence b is item b % 2 of the causal family (causal_pairs, single) at T = lens[b]. The output
    has total + 8 sentinel rows: every live row is written and meets the bar, nothing else changes --
    a grid smaller than the plan's tiles would leave sentinel rows among the live ones."""
    td = DT[dtype][0]
    W = _identity(td)
    for pattern in VARLEN_PATTERNS:
        lens = _varlen_lens(pattern, B, L)
        ids = P.ids_from_lens(lens, L, np.random.default_rng(7))
        plan, _ = _plan(ids, P.EOS)
        r_lens, r_offs, _, r_tiles, r_counts = P.reference(ids, P.EOS)
        assert (r_lens == lens).all() and (plan[0].cpu().numpy() == lens).all()
        assert (plan[3].cpu().numpy() == r_counts).all() and r_counts[1] <= P.tile_bound(B, L)
        total = int(r_counts[0])
        seq = np.repeat(np.arange(B), lens)
        parts = [_item_ref(family, int(t)) for t in lens]
        x = np.concatenate([q[b % 2] for b, (q, _) in enumerate(parts)])
        ref = np.concatenate([r[b % 2] for b, (_, r) in enumerate(parts)])
        X = _to_dev(x, td)
        out = torch.full((total + F.PAD_ROWS, F.LDO), F.SENTINEL, device="cuda").to(td)
        what = ("varlen", family, pattern, dtype, f"B {B}", f"L {L}", f"{r_counts[1]} tiles")
        assert _fused(dtype, True, X, W, None, out, B, L, F.H, K_ID, plan) == C.CLM_OK, what
        _hold_to_bar(out, total, ref, dtype, what,
                     lambda r: f"(sequence {seq[r]} of {lens[seq[r]]} rows, query {r - r_offs[seq[r]]})")


def _random_problem(td, rows, H, K, seed):
    """X [rows, ldx > K], W [3 d, ldw] scaled by K^-1/2 (its q rows by 1/8 as well), bias [3 d]"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    kr, d = (K + 63) // 64 * 64, H * 64
    X = torch.randn((rows, kr + 8), generator=g, device="cuda").to(td)
    W = torch.randn((3 * d, kr + 16), generator=g, device="cuda") / K ** 0.5
    W[:d] *= 0.125
    return X, W.to(td), torch.randn(3 * d, generator=g, device="cuda")


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("T", [1, 17, 50, 64, 65, 77, 128])
def test_fused_equals_gemm_plus_attention(dtype, causal, T):
    """kernels.hpp: "bit-identical to gemm(EPI_STORE) + attention()". Seeded randn X, W and bias with
    ldx > K, K in {64, 96, 128, 544, 768} (96 and 544: the half K-step), H in {1, 3}, B = G + 1: the
    whole output buffer, sentinel padding included, equals the two-kernel path's. Both of those kernels
    are held to torch references in test_gpu_kernels.py, so equality carries their bars over."""
    td = DT[dtype][0]
    B = 256 // T + 1
    for K in (64, 96, 128, 544, 768):
        for H in (1, 3):
            X, W, bias = _random_problem(td, B * T, H, K, 1000 * T + K + H)
            want = torch.full((B * T + 8, H * 64 + 64), -99.0, device="cuda").to(td)
            got = want.clone()
            _two_kernels(dtype, causal, X, W, bias, want, B, T, H, K)
            assert _fused(dtype, causal, X, W, bias, got, B, T, H, K) == C.CLM_OK, (K, H)
            assert (want[:B * T, :H * 64].float() != -99.0).all()
            assert torch.equal(got, want), (K, H, int((got != want).sum()))


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
@pytest.mark.parametrize("L", [16, 77, 128])
def test_fused_varlen_equals_fixed_length_rows(dtype, L):
    """what test_text_varlen_bit_identical claims at model level, on the kernel: sequence b's live rows
    of the packed run equal rows [0, lens[b]) of the fixed-length causal run on the padded batch, bit
    for bit; rows past the total keep the sentinel"""
    td = DT[dtype][0]
    B, H = 37, 3
    for pattern in ("random", "alternating"):
        lens = _varlen_lens(pattern, B, L)
        plan, rowmap = _plan(P.ids_from_lens(lens, L, np.random.default_rng(L)), P.EOS)
        total = int(lens.sum())
        rm = rowmap[:total].long()
        assert (rm.cpu().numpy() == P.reference(P.ids_from_lens(lens, L, np.random.default_rng(L)), P.EOS)[2]).all()
        for K in (128, 544):
            X, W, bias = _random_problem(td, B * L, H, K, L + K)
            padded = torch.full((B * L, H * 64 + 64), -99.0, device="cuda").to(td)
            assert _fused(dtype, True, X, W, bias, padded, B, L, H, K) == C.CLM_OK
            Xp = X[rm].contiguous()
            packed = torch.full((total + 8, H * 64 + 64), -99.0, device="cuda").to(td)
            assert _fused(dtype, True, Xp, W, bias, packed, B, L, H, K, plan) == C.CLM_OK
            assert torch.equal(packed[:total], padded[rm]), (pattern, K)
            assert (packed[total:].float() == -99.0).all() and (packed[:total, :H * 64].float() != -99.0).all()


def test_fused_refusals_write_nothing():
    """T = 129, K = 48, ldx % 8 != 0, ldo < d, varlen with B > 65535, a partial plan: an error each, the
    output untouched; the next call works"""
    X, W, bias = _random_problem(torch.float16, 300, 1, 64, 5)
    out = torch.full((300, 128), -99.0, device="cuda").half()
    plan, _ = _plan(P.ids_from_lens(np.full(4, 16), 16, np.random.default_rng(0)), P.EOS)
    lens, offs, tiles, counts = plan
    run = functools.partial(_fused, "float16")
    refused = [
        run(False, X, W, bias, out, 2, 129, 1, 64),
        run(False, X, W, bias, out, 4, 16, 1, 48),
        run(False, X, W, bias, out, 4, 16, 1, 64, ldx=X.stride(0) + 4),
        run(False, X, W, bias, out, 4, 16, 1, 64, ldo=60),
        run(True, X, W, bias, out, 65536, 16, 1, 64, plan),
        run(True, X, W, bias, out, 4, 16, 1, 64, (lens, offs, tiles, None)),
        run(True, X, W, bias, out, 4, 16, 1, 64, (None, None, None, counts)),
        run(False, X, W, bias, out, 4, 16, 1, 64, (lens, None, None, None)),
    ]
    torch.cuda.synchronize()
    assert all(rc != C.CLM_OK for rc in refused), refused
    assert refused[5] == refused[6] == refused[7] == C.CLM_E_ARG
    assert (out.float() == -99.0).all()
    assert run(True, X, W, bias, out, 4, 16, 1, 64, plan) == C.CLM_OK
    torch.cuda.synchronize()
    assert (out[:64, :64].float() != -99.0).all() and (out[64:].float() == -99.0).all()


def _poisons(dtype):
    """NaN, and a finite 16-bit value whose projections overflow to Inf"""
    return {"nan": float("nan"), "inf": 60000.0 if dtype == "float16" else 3.0e38}


def _others_unchanged(clean, got, row_ranges, skip):
    """names of the sequences other than `skip` whose rows differ from the clean run"""
    return [b for b, (r0, r1) in enumerate(row_ranges) if b != skip and not torch.equal(got[r0:r1], clean[r0:r1])]


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("T", [50, 77, 100])
def test_fused_isolates_non_finite_sequences_fixed(dtype, causal, T):
    """One sequence's X rows set to NaN, or to a value that makes its V overflow to Inf; the sequence
    in the middle of a tile, last in a tile and first in the next tile in turn. Every other sequence's
    output equals the clean run bit for bit (the poisoned one's own rows are unconstrained): an item's
    embedding must not depend on its batch neighbours. clm_gemm + clm_attention on the same input is
    the control.

    This test found the fused kernel multiplying P = 0 of the masked keys past a sequence's end with
    the *next* sequence's V rows (v_frag_rows clamped to the tile, not the sequence): 0 x NaN and
    0 x Inf are NaN, so the predecessor of a non-finite sequence came out NaN as well, while the
    two-kernel path (attn_small_kernel zero-fills V past T) kept it clean."""
    td = DT[dtype][0]
    G, H, K = 256 // T, 3, 128
    B = 2 * G + 1
    X, W, bias = _random_problem(td, B * T, H, K, T)
    rows = [(b * T, (b + 1) * T) for b in range(B)]

    def both(x):
        a = torch.full((B * T, H * 64), -99.0, device="cuda").to(td)
        b = a.clone()
        assert _fused(dtype, causal, x, W, bias, a, B, T, H, K) == C.CLM_OK
        return a, b, _two_kernels(dtype, causal, x, W, bias, b, B, T, H, K)

    clean, clean2, _ = both(X)
    assert torch.equal(clean, clean2) and torch.isfinite(clean.float()).all()
    failures = []
    for name, s in (("middle of a tile", G // 2 if G > 2 else None), ("last in a tile", G - 1), ("first in a tile", G)):
        if s is None:
            continue
        for kind, value in _poisons(dtype).items():
            x = X.clone()
            x[s * T:(s + 1) * T] = value
            got, got2, qkv = both(x)
            v = qkv[s * T:(s + 1) * T, 2 * H * 64:].float().reshape(T, H, 64)
            assert (torch.isnan(v) if kind == "nan" else torch.isinf(v)).any(-1).all(), (name, kind)
            assert not _others_unchanged(clean2, got2, rows, s), ("the two-kernel control", name, kind)
            hit = _others_unchanged(clean, got, rows, s)
            if hit:
                failures.append((name, kind, f"sequence {s}", f"changed sequences {hit}"))
    assert not failures, failures


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_fused_isolates_non_finite_sequences_varlen(dtype):
    """the same over packed sequences (L = 77, 37 captions of seeded random lengths, causal): the
    poisoned sequence in the middle of a tile, last in a tile and first in a tile of clm_text_plan's
    plan; the control is the fixed-length two-kernel path on the padded batch."""
    td = DT[dtype][0]
    B, L, H, K = 37, 77, 3, 128
    lens = _varlen_lens("random", B, L)
    ids = P.ids_from_lens(lens, L, np.random.default_rng(1))
    plan, rowmap = _plan(ids, P.EOS)
    _, offs, _, tiles, counts = P.reference(ids, P.EOS)
    assert counts[1] >= 3
    total = int(counts[0])
    rm = rowmap[:total].long()
    first, n = int(tiles[1] & 0xFFFF), int(tiles[1] >> 16)
    assert n >= 3
    X, W, bias = _random_problem(td, B * L, H, K, 11)
    rows = [(int(offs[b]), int(offs[b + 1])) for b in range(B)]

    def both(x):
        a = torch.full((total, H * 64), -99.0, device="cuda").to(td)
        b = torch.full((B * L, H * 64), -99.0, device="cuda").to(td)
        assert _fused(dtype, True, x[rm].contiguous(), W, bias, a, B, L, H, K, plan) == C.CLM_OK
        _two_kernels(dtype, True, x, W, bias, b, B, L, H, K)
        return a, b[rm]

    clean, clean2 = both(X)
    assert torch.equal(clean, clean2) and torch.isfinite(clean.float()).all()
    failures = []
    for name, s in (("middle of a tile", first + n // 2), ("last in a tile", first + n - 1), ("first in a tile", first)):
        for kind, value in _poisons(dtype).items():
            x = X.clone()
            x[s * L:(s + 1) * L] = value
            got, got2 = both(x)
            assert not _others_unchanged(clean2, got2, rows, s), ("the two-kernel control", name, kind)
            hit = _others_unchanged(clean, got, rows, s)
            if hit:
                failures.append((name, kind, f"sequence {s}", f"changed sequences {hit}"))
    assert not failures, failures
