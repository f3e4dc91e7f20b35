"""The index passes' selecting GEMM epilogues (gemm_common.hpp: EPI_FILTER, EPI_FILTER_MASK, EPI_RANK,
EPI_LSE) through clm_gemm_select, on every tile config that has them, and clm_value_bounds, which makes
the skip test's cbound keys. The index endpoints re-score candidates exactly and redo overflowed lists,
so a wrong epilogue (a column appended twice or wrongly, one dropped outside the true top-k, a miscount
past cap, a tail partial in a neighbour's slot) does not show there; here every list, count and slab
slot is compared directly.

Which tile the endpoints' tests reach. pick_config sends all four epilogues to the G2 cost model
(k_gemm.hip pick_from(MODELS_G2)): cost = ceil(tiles / 256) * bm * bn / eff. While one round covers the
grid that is 19.1 k / 13.9 k / 19.5 k / 14.0 k for configs 8 / 9 / 10 / 11, so config 9 (256 x 128) runs
at the parametrised shapes of test_gpu_rank.py, test_gpu_lse.py, test_gpu_masked_search.py and
test_gpu_range.py: N = 1 .. 9000 rows x up to 300 queries, and the 1300-query blocks x 1000 rows of their
nq = 2600 cases. _g2_pick below is a copy of the model, kept in step by hand; tests/test_gemm_select_host.py
holds its table against the MODELS_G2 line of k_gemm.hip and pins these figures. The model's
other picks: config 11 (128 x 256) for the masked suite's two large cases (70,001 and 40,999 rows x 300),
for 300,000 rows x <= 128 queries and for this file's persistent case (70,000 x 70); config 8
(256 x 192) at the benchmark's 10 M rows x 512 queries (407 rounds x 19.1 k against 611 x 13.9 k for
config 9). Config 1 runs only where the search asks for it (its dense and overflow passes). So without
this file RANK, LSE and FILTER_MASK on configs 1, 8 and 10, and all but a few cases on 11 -- among them
the tile the large index runs -- were untested.

Two oracles, used together.
  * Bitwise: S = clm_gemm(CLM_EPI_SCORE) on the same config, fp32 (checked against torch by
    test_gemm_epilogues_vs_torch). The epilogues compute acc * rscale[m] * cscale[n] in the same order,
    so membership is decided exactly by S and fp32 arithmetic on theta and margin (lo = theta - margin,
    hi = theta + margin in torch.float32): each row's list is exactly the passing columns as a multiset,
    each id is base + n, each cand_s is S[m, n] bit for bit, cnt is the true count stored or not, above
    is #{S > hi}.
  * Independent: fp64 scores D from the fp16 operands and fp32 scales. Every pair farther from each
    decision edge than E[m, n] = (K + 2) 2^-23 |rscale[m] cscale[n]| sum_k |a_k w_k| (the fp32 dot
    product bound, doubled for the unknown MFMA summation order) must be decided as fp64 decides it; at
    most 0.5 % of a case's pairs may lie inside E (asserted). The inputs are drawn on the CPU from fixed
    seeds; with the sweep's thresholds (_thresholds) at most 0.006 % of a case's pairs lie there, with
    the persistent case's 0.002 %.

LSE slab. Slot j of a row holds the tail sum of the columns [j w, (j + 1) w), w = the config's wave
column extent (128 / 96 / 64 / 64 / 64 for configs 1 / 8 / 9 / 10 / 11). Reference: the fp64 sum of
exp2((S[m, n] - theta) * lse_c) over that extent's non-band columns. Bound, relative to the reference
slot sum: ln2 * max|arg| * 2^-23 (the fp32 argument: one rounding each in the subtraction and the
product) + 2^-23 (the hardware exp2, 1 ulp) + (w + 2) * 2^-24 (at most w + 2 positive fp32 additions),
with max|arg| taken from the case; arguments stay >= -64 so no term is flushed. Measured on the MI355X:
see test_sweep's docstring.
"""
import functools
import math

import numpy as np
import pytest
import torch

from clip_lora_match_amd import _capi as C

pytestmark = pytest.mark.gpu

FILTER, RANK, LSE, MASK = C.CLM_EPI_FILTER, C.CLM_EPI_RANK, C.CLM_EPI_LSE, C.CLM_EPI_FILTER_MASK
EPIS = {"FILTER": FILTER, "RANK": RANK, "LSE": LSE, "FILTER_MASK": MASK}
G2_CFGS = [1, 8, 9, 10, 11]          # the tiles RANK / LSE / FILTER_MASK exist on
FILTER_CFGS = list(range(13))        # FILTER: every gemm_kernel / G2 tile; 13 / 14 (G4) have no such epilogue
TILE = {1: (256, 256, 2), 8: (256, 192, 2), 9: (256, 128, 2), 10: (192, 256, 4), 11: (128, 256, 4)}   # BM, BN, WN
G2_MODEL = {8: (256, 192, 2.569), 9: (256, 128, 2.349), 10: (192, 256, 2.521), 11: (128, 256, 2.340)}
S_SENT, I_SENT, C_SENT, A_SENT = -99.0, -12345, -7, 0x5A5A5A5A
BIG_BASE = (1 << 32) + 12345
LSE_C = 2.5


def _cfgs_of(epi):
    return FILTER_CFGS if epi == FILTER else G2_CFGS


def _g2_pick(M, N):
    """pick_from(MODELS_G2, M, N) of k_gemm.hip"""
    best, best_cost = 8, 1e300
    for cid, (bm, bn, eff) in G2_MODEL.items():
        tiles = -(-M // bm) * -(-N // bn)
        cost = -(-tiles // 256) * bm * bn / eff
        if cost < best_cost * 0.999:
            best, best_cost = cid, cost
    return best


def _p(t):
    return C.ptr(t) if t is not None else None


def _st():
    return C.stream_of(torch.device("cuda:0"))


def _i32(t):
    return t.contiguous().view(torch.int32)


def _scores(cfg, A, W, rs, cs):
    """the bitwise oracle: the fp32 score matrix of the same config. cfg = -1: of the tile the selecting
    epilogues' heuristic picks (_g2_pick) -- clm_gemm's own -1 would pick among the encoder's tiles,
    and match only because every tile sums K in the same order"""
    M, K = A.shape
    N = W.shape[0]
    cfg = cfg if cfg >= 0 else _g2_pick(M, N)
    S = torch.empty((M, N), dtype=torch.float32, device="cuda")
    C.check(C.lib().clm_gemm(0, C.CLM_F16, C.CLM_EPI_SCORE, cfg, C.ptr(A), A.stride(0), C.ptr(W), W.stride(0), M, N, K,
                             C.ptr(S), S.stride(0), None, _p(rs), _p(cs), _st()), "clm_gemm")
    return S


def _bounds(cs):
    keys = torch.zeros(2, dtype=torch.int32, device="cuda")
    C.check(C.lib().clm_value_bounds(0, C.ptr(cs), cs.numel(), C.ptr(keys), _st()), "clm_value_bounds")
    return keys


def _mask_words(allowed):
    """bool [N] (CPU or device) -> ceil(N / 32) little-endian words on the device"""
    a = allowed.cpu().numpy().astype(np.uint8)
    b = np.packbits(a, bitorder="little")
    b = np.concatenate([b, np.zeros(-len(b) % 4, dtype=np.uint8)])
    return torch.from_numpy(b.view(np.int32).copy()).cuda()


class Run:
    """one clm_gemm_select call into sentinel-filled buffers two rows taller than M"""

    def __init__(self, epi, cfg, A, W, rs, cs, theta, margin=0.0, cap=None, base=0, cbound=None, mask=None,
                 m_fastest=1, lse_c=LSE_C, expect=C.CLM_OK):
        M, K = A.shape
        N = W.shape[0]
        self.epi, self.M, self.N, self.base = epi, M, N, base
        self.cap = cap = N if cap is None else cap
        self.cnt = torch.full((M + 2,), C_SENT, dtype=torch.int32, device="cuda")
        self.cnt[:M] = 0
        self.above = torch.full((M + 2,), A_SENT, dtype=torch.int32, device="cuda")
        self.above[:M] = 0
        self.cand_s = torch.full((M + 2, cap), S_SENT, dtype=torch.float32, device="cuda")
        self.cand_i = torch.full((M + 2, cap), I_SENT, dtype=torch.int64, device="cuda")
        self.lse_ld = N // 64 + 4 + 3
        self.slab = torch.full((M + 2, self.lse_ld), S_SENT, dtype=torch.float32, device="cuda")
        th = theta if theta.dim() == 2 else theta[:, None]
        self.rc = C.lib().clm_gemm_select(
            0, epi, cfg, C.ptr(A), A.stride(0), C.ptr(W), W.stride(0), M, N, K, _p(rs), _p(cs), C.ptr(th),
            th.stride(0), margin, C.ptr(self.cnt), C.ptr(self.cand_s), C.ptr(self.cand_i), cap, base, _p(cbound),
            C.ptr(self.above), C.ptr(self.slab), self.lse_ld, lse_c, _p(mask), m_fastest, _st())
        assert self.rc == expect, (self.rc, C.lib().clm_last_error())

    def untouched(self):
        M = self.M
        return bool((self.cnt[:M] == 0).all() and (self.cnt[M:] == C_SENT).all() and (self.above[:M] == 0).all()
                    and (self.above[M:] == A_SENT).all() and (self.cand_s == S_SENT).all()
                    and (self.cand_i == I_SENT).all() and (self.slab == S_SENT).all())

    def dense(self):
        """(times[M, N] = how often column n is stored in row m's list, bits[M, N] = the stored cand_s
        bits, 0 where none), after checking the slot discipline: the first min(cnt, cap) slots of a live
        row hold ids base + n with 0 <= n < N, every other slot and the rows at or past M are untouched"""
        M, N, cap = self.M, self.N, self.cap
        assert (self.cnt[M:] == C_SENT).all() and (self.cnt[:M] >= 0).all()
        assert (self.cand_i[M:] == I_SENT).all() and (self.cand_s[M:] == S_SENT).all()
        used = torch.arange(cap, device="cuda")[None, :] < self.cnt[:M, None].clamp(max=cap)
        ci, csb = self.cand_i[:M], self.cand_s[:M]
        assert (ci[~used] == I_SENT).all() and (csb[~used] == S_SENT).all(), "a slot at or past min(cnt, cap) written"
        n = ci - self.base
        assert ((n >= 0) & (n < N))[used].all(), "a stored id is not base + n"
        if self.epi in (RANK, LSE):
            assert (csb == S_SENT).all(), "RANK / LSE wrote cand_s"
        nn = torch.where(used, n, torch.full_like(n, N))   # unused slots go to a spare column N
        times = torch.zeros((M, N + 1), dtype=torch.int32, device="cuda").scatter_add_(1, nn, used.int())[:, :N]
        bits = torch.zeros((M, N + 1), dtype=torch.int32, device="cuda")
        if self.epi in (FILTER, MASK):   # a column stored twice shows in `times`; its bits are then either entry's
            bits.scatter_(1, nn, torch.where(used, _i32(csb), torch.zeros_like(nn, dtype=torch.int32)))
        bits = bits[:, :N]
        return times, bits


def _edges(theta, margin):
    """lo / hi as the epilogues compute them: fp32"""
    t = (theta if theta.dim() == 1 else theta[:, 0]).float()
    m = torch.tensor(margin, dtype=torch.float32, device=t.device)
    return t - m, t + m


def _members(epi, S, theta, margin, allowed=None):
    """(listed[M, N], above[M]) decided by the bitwise oracle"""
    lo, hi = _edges(theta, margin)
    t = theta if theta.dim() == 1 else theta[:, 0]
    if epi == FILTER:
        return S >= t[:, None], None
    if epi == MASK:
        return (S >= t[:, None]) & allowed[None, :].to(S.device), None
    if epi == LSE:
        return S >= lo[:, None], None
    up = S > hi[:, None]
    return (S >= lo[:, None]) & ~up, up.sum(1).int()


def check_bitwise(r, S, theta, margin=0.0, allowed=None):
    """every list, count and `above` against S; returns (times, bits) for further comparisons"""
    M = r.M
    listed, up = _members(r.epi, S, theta, margin, allowed)
    true_cnt = listed.sum(1).int()
    times, bits = r.dense()
    assert torch.equal(r.cnt[:M], true_cnt), "cnt is not the true count"
    over = true_cnt > r.cap
    assert (times <= listed.int()).all(), "a column listed twice, or one that does not pass"
    assert torch.equal(times.sum(1).int(), true_cnt.clamp(max=r.cap))
    assert torch.equal(times[~over], listed[~over].int()), "a passing column is missing"
    if r.epi in (FILTER, MASK):
        assert torch.equal(bits, torch.where(times > 0, _i32(S), torch.zeros_like(bits))), "cand_s is not S[m, n]"
    if r.epi == RANK:
        assert torch.equal(r.above[:M], up), "above is not #{S > hi}"
        assert (r.above[M:] == A_SENT).all()
    else:
        assert (r.above[:M] == 0).all() and (r.above[M:] == A_SENT).all()
    if r.epi != LSE:
        assert (r.slab == S_SENT).all()
    return times, bits


def check_independent(r, times, D, E, theta, margin=0.0, allowed=None):
    """pairs farther than E from every decision edge are decided as fp64 decides them"""
    lo, hi = _edges(theta, margin)
    lo, hi = lo.double()[:, None], hi.double()[:, None]
    t = (theta if theta.dim() == 1 else theta[:, 0]).double()[:, None]
    if r.epi in (FILTER, MASK):
        clear, want = (D - t).abs() > E, D >= t
        if r.epi == MASK:
            want = want & allowed[None, :].to(D.device)
    elif r.epi == LSE:
        clear, want = (D - lo).abs() > E, D >= lo
    else:
        clear = ((D - lo).abs() > E) & ((D - hi).abs() > E)
        want = (D >= lo) & (D <= hi)
        up = r.above[:r.M].long()
        assert (up >= ((D > hi) & clear).sum(1)).all() and (up <= ((D > hi) | ~clear).sum(1)).all()
    frac = 1.0 - clear.double().mean().item()
    assert frac <= 0.005, f"{frac:.4%} of the pairs lie within E of an edge: the independent oracle is too thin"
    assert torch.equal((times > 0)[clear], want[clear]), "a pair clear of every edge is decided against fp64"
    return frac


def check_slab(r, cfg, S, theta, margin, lse_c=LSE_C):
    """every slot of the live rows against the fp64 tail sum of its wave-column extent"""
    M, N = r.M, r.N
    _, bn, wn = TILE[cfg if cfg >= 0 else _g2_pick(M, N)]
    w = bn // wn
    nslots = -(-N // bn) * wn
    assert nslots <= N // 64 + 4
    assert (r.slab[M:] == S_SENT).all() and (r.slab[:M, nslots:] == S_SENT).all(), "a slot outside the prefix written"
    lo, _ = _edges(theta, margin)
    t = (theta if theta.dim() == 1 else theta[:, 0]).double()[:, None]
    tail = ~(S >= lo[:, None])
    arg = (S.double() - t) * lse_c
    assert arg[tail].numel() == 0 or arg[tail].min() >= -64.0
    terms = torch.where(tail, torch.exp2(arg), torch.zeros_like(arg))
    pad = nslots * w - N
    ref = torch.nn.functional.pad(terms, (0, pad)).view(M, nslots, w).sum(2)
    amax = float(arg[tail].abs().max()) if arg[tail].numel() else 0.0
    bound = math.log(2.0) * amax * 2.0 ** -23 + 2.0 ** -23 + (w + 2) * 2.0 ** -24
    got = r.slab[:M, :nslots].double()
    err = (got - ref).abs()
    rel = float((err / ref.clamp(min=1e-300))[ref > 0].max()) if bool((ref > 0).any()) else 0.0
    assert (err <= bound * ref).all(), f"slot error {rel:.3e} above the bound {bound:.3e}"
    return rel


# ------------------------------------------------------------------------------------ inputs -----
@functools.lru_cache(maxsize=None)
def _cpu_inputs(M, N, K):
    g = torch.Generator().manual_seed(100003 * M + 101 * N + K)
    A = torch.randn((M, K), generator=g).half()
    W = (torch.randn((N, K), generator=g) / K ** 0.5).half()
    rs = torch.rand(M, generator=g) + 0.5
    cs = torch.rand(N, generator=g) + 0.5
    return A, W, rs, cs


def _ref64(A, W, rs, cs):
    """(D, E): fp64 scores and the fp32 GEMM's error bound around them"""
    K = A.shape[1]
    sc = rs.double()[:, None] * cs.double()[None, :]
    D = (A.double() @ W.double().T) * sc
    E = (K + 2) * 2.0 ** -23 * sc.abs() * (A.double().abs() @ W.double().abs().T)
    return D, E


def _thresholds(D, E):
    """even rows: the row's median, odd rows: its 99th percentile, each halfway between the two scores
    around it, then moved by at most 0.032 (17 candidates 0.004 apart, far more than E) to where the
    three edges theta, theta - MARGIN and theta + MARGIN lie farthest, in units of E, from the row's
    scores: with 4 columns a threshold of a given rank is otherwise within E of a score in about one
    row of a hundred, more than the 0.5 % the independent oracle may leave undecided"""
    q = torch.quantile(D, torch.tensor([0.5, 0.99], dtype=D.dtype, device=D.device), dim=1, interpolation="midpoint")
    odd = (torch.arange(D.shape[0], device=D.device) % 2).bool()
    base = torch.where(odd, q[1], q[0])
    offs = torch.arange(-8, 9, dtype=D.dtype, device=D.device) * 0.004
    cand = (base[None, :] + offs[:, None]).float()   # [17, M]
    m32 = torch.tensor(MARGIN, dtype=torch.float32, device=D.device)
    room = None
    for edge in (cand, cand - m32, cand + m32):
        r = ((D[None] - edge.double()[:, :, None]).abs() / E[None]).amin(2)
        room = r if room is None else torch.minimum(room, r)
    pick = room.argmax(0)
    return cand[pick, torch.arange(D.shape[0], device=D.device)].contiguous()


@functools.lru_cache(maxsize=None)
def _case(M, N, K):
    A, W, rs, cs = (t.cuda() for t in _cpu_inputs(M, N, K))
    D, E = _ref64(A, W, rs, cs)
    theta = _thresholds(D, E)
    g = torch.Generator().manual_seed(N)
    allowed = (torch.rand(N, generator=g) < 0.5).cuda()
    return A, W, rs, cs, D, E, theta, allowed, _mask_words(allowed)


MARGIN = 0.05   # RANK / LSE: a band of a few per cent of the columns around a median threshold


def _run_checked(epi, cfg, M, N, K, m_fastest=1, cbound=False, base=0):
    A, W, rs, cs, D, E, theta, allowed, words = _case(M, N, K)
    margin = MARGIN if epi in (RANK, LSE) else 0.0
    S = _scores(cfg, A, W, rs, cs)
    r = Run(epi, cfg, A, W, rs, cs, theta, margin, base=base, cbound=_bounds(cs) if cbound else None,
            mask=words if epi == MASK else None, m_fastest=m_fastest)
    times, bits = check_bitwise(r, S, theta, margin, allowed)
    check_independent(r, times, D, E, theta, margin, allowed)
    if epi == LSE:
        check_slab(r, cfg, S, theta, margin)
    return r, times, bits


# ------------------------------------------------------------------------------------- sweep -----
SWEEP = [(name, cfg) for name, epi in EPIS.items() for cfg in _cfgs_of(epi) + [-1]]


@pytest.mark.parametrize("K", [64, 192, 512])
@pytest.mark.parametrize("name,cfg", SWEEP)
def test_sweep(name, cfg, K):
    """M = 1 / 70 (below every tile height) / 300 (2 or 3 ragged row tiles, both tile orders) x N = 4 /
    64 / 1000 (a ragged last tile for 128, 192 and 256) / 1003 (the scalar path), against both oracles;
    LSE also slot by slot. The skip test is on for M = 70 and off elsewhere (test_skip_* compares the two).
    Largest LSE slot error measured on the MI355X over this sweep: 4.1e-07 of the slot sum (M = 300,
    N = 4, the same on every config), against bounds of 9.1e-06 / 7.2e-06 / 5.3e-06 there for w =
    128 / 96 / 64; over the whole file 4.1e-07 as well (persistent case: 3.3e-07 against 7.3e-06)."""
    epi = EPIS[name]
    for M, mf in ((1, 1), (70, 1), (300, 0), (300, 1)):
        for N in (4, 64, 1000, 1003):
            _run_checked(epi, cfg, M, N, K, m_fastest=mf, cbound=(M == 70))


@pytest.mark.parametrize("name", list(EPIS))
def test_refused_configs_write_nothing(name):
    """FILTER has no G4 form (configs 13 / 14), the others exist on 1 and 8-11 only: CLM_E_HIP, and not
    one byte of any output written; a config past the table is CLM_E_ARG"""
    epi = EPIS[name]
    A, W, rs, cs, D, E, theta, allowed, words = _case(70, 1000, 64)
    for cfg in range(C.lib().clm_gemm_num_configs()):
        if cfg in _cfgs_of(epi):
            continue
        r = Run(epi, cfg, A, W, rs, cs, theta, MARGIN, mask=words, expect=C.CLM_E_HIP)
        assert r.untouched(), cfg
    r = Run(epi, C.lib().clm_gemm_num_configs(), A, W, rs, cs, theta, MARGIN, mask=words, expect=C.CLM_E_ARG)
    assert r.untouched()


@pytest.mark.parametrize("name", list(EPIS))
def test_persistent_grid(name):
    """M = 70, N = 70,000, K = 64: every config has more tiles than the 256 CUs, so workgroups walk
    several tiles. Lists, counts and slab equal the one-tile-per-workgroup run (clm_debug_set(4)) and
    both oracles hold."""
    epi = EPIS[name]
    M, N, K = 70, 70_000, 64
    A, W, rs, cs = (t.cuda() for t in _cpu_inputs(M, N, K))
    D, E = _ref64(A, W, rs, cs)
    theta = torch.quantile(D, 0.995, dim=1).float()
    margin = 0.01 if epi in (RANK, LSE) else 0.0
    allowed = (torch.rand(N, generator=torch.Generator().manual_seed(7)) < 0.5).cuda()
    words = _mask_words(allowed)
    keys = _bounds(cs)
    for cfg in _cfgs_of(epi) + [-1]:
        S = _scores(cfg, A, W, rs, cs)
        res = []
        try:
            for dbg in (0, 4):
                C.lib().clm_debug_set(dbg)
                r = Run(epi, cfg, A, W, rs, cs, theta, margin, cap=1024, cbound=keys, mask=words)
                times, bits = check_bitwise(r, S, theta, margin, allowed)
                res.append((r, times, bits))
        finally:
            C.lib().clm_debug_set(0)
        (r0, t0, b0), (r1, t1, b1) = res
        assert torch.equal(t0, t1) and torch.equal(b0, b1) and torch.equal(r0.cnt, r1.cnt)
        assert torch.equal(r0.above, r1.above) and torch.equal(_i32(r0.slab), _i32(r1.slab))
        check_independent(r0, t0, D, E, theta, margin, allowed)
        if epi == LSE:
            check_slab(r0, cfg, S, theta, margin)


# ------------------------------------------------------------------------------------- edges -----
def _lattice(M, N, K=64):
    """operands in {-2 .. 2} and power-of-two scales: every score is an exact multiple of 1/4, so
    thresholds and margins on that lattice meet many scores exactly"""
    g = torch.Generator().manual_seed(M * 31 + N)
    A = torch.randint(-2, 3, (M, K), generator=g).half().cuda()
    W = torch.randint(-2, 3, (N, K), generator=g).half().cuda()
    rs = torch.full((M,), 0.25, device="cuda")
    cs = torch.ones(N, device="cuda")
    return A, W, rs, cs


def _both_ways(epi, cfg, A, W, rs, cs, S, theta, margin, allowed=None, lse_c=LSE_C):
    """the run without cbound and the one with it (the branch every index pass takes), each against S,
    and equal to each other; returns the cbound run's (times, bits)"""
    words = _mask_words(allowed) if allowed is not None else None
    out = []
    for keys in (None, _bounds(cs)):
        r = Run(epi, cfg, A, W, rs, cs, theta, margin, cbound=keys, mask=words, lse_c=lse_c)
        out.append((r,) + check_bitwise(r, S, theta, margin, allowed))
    assert _same(*out[0], *out[1]), "the skip test changed a result"
    return out[1][1], out[1][2]


@pytest.mark.parametrize("N", [1000, 1003])
@pytest.mark.parametrize("cfg", G2_CFGS)
def test_ties(cfg, N):
    """a threshold that is a score bit for bit, with the skip test off and on (FILTER's two vector
    branches): FILTER's >= lists it; RANK with margin 0 counts only S > t and lists S == t; RANK with a
    margin whose edges both meet scores: S == hi and S == lo are band entries, not counted. With the
    threshold at the row's largest score and cscale = 1 the skip bound of that score's 16 x 16 block
    equals the threshold, so the skip predicate's own >= decides whether the row lists anything; the
    same with every score <= 0 (the cmin side of the bound)."""
    M = 70
    A, W, rs, cs = _lattice(M, N)
    S = _scores(cfg, A, W, rs, cs)
    assert (S * 4 == (S * 4).round()).all()
    theta = S.sort(1, descending=True).values[:, 400].contiguous()   # each row's 401st largest, ties included
    allowed = torch.ones(N, dtype=torch.bool)
    allowed[::3] = False
    for epi, margin in ((FILTER, 0.0), (MASK, 0.0), (RANK, 0.0), (RANK, 1.5), (LSE, 1.5)):
        times, _ = _both_ways(epi, cfg, A, W, rs, cs, S, theta, margin, allowed, lse_c=1.0)
        lo, hi = _edges(theta, margin)
        at_lo, at_hi = S == lo[:, None], S == hi[:, None]
        assert at_lo.any(1).all() and at_hi.any(1).all(), "the case must meet both edges in every row"
        if epi == MASK:
            at_lo, at_hi = at_lo & allowed.cuda()[None, :], at_hi & allowed.cuda()[None, :]
        if epi == RANK:
            assert (times[at_hi] == 1).all(), "a score equal to hi belongs to the band"
        assert (times[at_lo] == 1).all(), "a score equal to the lower edge is listed"
    # the threshold at the row's largest score: only the blocks that hold it may pass the skip test,
    # and their bound equals the threshold. Then the same with every accumulator <= 0.
    ones = torch.ones(N, dtype=torch.bool)
    for A2, W2 in ((A, W), (-A.abs(), W.abs())):
        S2 = _scores(cfg, A2, W2, rs, cs)
        top = S2.max(1).values.contiguous()
        assert ((S2 == top[:, None]).sum(1) >= 1).all() and (S2 <= top[:, None]).all()
        for epi in (FILTER, MASK, RANK):
            times, _ = _both_ways(epi, cfg, A2, W2, rs, cs, S2, top, 0.0, ones)
            assert torch.equal(times, (S2 == top[:, None]).int()), "exactly the row's largest scores are listed"
    # Gaussian scores: one tie per row, the threshold taken from S itself
    A, W, rs, cs, D, E, _, _, _ = _case(M, N, 64)
    S = _scores(cfg, A, W, rs, cs)
    col = torch.arange(M, device="cuda") * 13 % N
    theta = S[torch.arange(M, device="cuda"), col].contiguous()
    for epi in (FILTER, MASK, RANK):
        times, _ = _both_ways(epi, cfg, A, W, rs, cs, S, theta, 0.0, ones)
        assert (times[torch.arange(M, device="cuda"), col] == 1).all()


@pytest.mark.parametrize("N", [1000, 1003])
@pytest.mark.parametrize("name", list(EPIS))
def test_capacity(name, N):
    """cap = 8 of about 30 passing columns: cnt is the full count, the 8 stored entries are distinct
    members of the true set, nothing past slot 8 or at / past row M is touched (check_bitwise / dense)"""
    epi = EPIS[name]
    M = 70
    A, W, rs, cs, D, E, _, _, _ = _case(M, N, 64)
    # about 30 at or above the 97th percentile; RANK: a band of about 50 around the 90th
    theta = torch.quantile(D, 0.9 if epi == RANK else 0.97, dim=1).float()
    margin = {RANK: 0.15, LSE: 0.05}.get(epi, 0.0)
    allowed = torch.ones(N, dtype=torch.bool)
    for cfg in G2_CFGS:
        S = _scores(cfg, A, W, rs, cs)
        r = Run(epi, cfg, A, W, rs, cs, theta, margin, cap=8, mask=_mask_words(allowed))
        times, _ = check_bitwise(r, S, theta, margin, allowed)
        assert (r.cnt[:M] > 8).all() and (times.sum(1) == 8).all()
        r1 = Run(epi, cfg, A, W, rs, cs, theta, margin, cap=1, mask=_mask_words(allowed))
        check_bitwise(r1, S, theta, margin, allowed)


@pytest.mark.parametrize("N", [1000, 1003])
@pytest.mark.parametrize("name", list(EPIS))
def test_big_base_and_theta_stride(name, N):
    """ids are 64-bit (base above 2^32), and thresholds are read with their stride: column 0 of a
    [M, 3] array whose other columns would select everything or nothing"""
    epi = EPIS[name]
    M = 70
    A, W, rs, cs, D, E, theta, allowed, words = _case(M, N, 64)
    wide = torch.stack([theta, torch.full_like(theta, -1e30), torch.full_like(theta, float("nan"))], dim=1).contiguous()
    margin = MARGIN if epi in (RANK, LSE) else 0.0
    for cfg in G2_CFGS:
        S = _scores(cfg, A, W, rs, cs)
        r = Run(epi, cfg, A, W, rs, cs, wide, margin, base=BIG_BASE, mask=words)
        times, bits = check_bitwise(r, S, wide, margin, allowed)
        r0 = Run(epi, cfg, A, W, rs, cs, theta, margin, mask=words)
        t0, b0 = check_bitwise(r0, S, theta, margin, allowed)
        assert torch.equal(times, t0) and torch.equal(bits, b0) and torch.equal(r.cnt, r0.cnt)
        used = torch.arange(r.cap, device="cuda")[None, :] < r.cnt[:M, None]
        assert (r.cand_i[:M][used] >= BIG_BASE).all()


def _same(ra, ta, ba, rb, tb, bb):
    return (torch.equal(ta, tb) and torch.equal(ba, bb) and torch.equal(ra.cnt, rb.cnt)
            and torch.equal(ra.above, rb.above) and torch.equal(_i32(ra.slab), _i32(rb.slab)))


@functools.lru_cache(maxsize=None)
def _skip_scenarios():
    """(name, A, W, rs, cs, theta): M = 70, N = 1000, K = 64 (the vector path: the skip test's)"""
    M, N, K = 70, 1000, 64
    A, W, rs, cs, D, E, _, _, _ = _case(M, N, K)
    g = torch.Generator().manual_seed(5)
    out = [("high thresholds", A, W, rs, cs, torch.quantile(D, 0.999, dim=1).float())]
    # every accumulator negative, cscale over 4 decades: the passing columns are those with a small
    # cscale, which only the cmin side of the bound admits
    An, Wn = -A.abs(), W.abs()
    cs4 = (10.0 ** (torch.rand(N, generator=g) * 4 - 3)).cuda()
    Dn, _ = _ref64(An, Wn, rs, cs4)
    out.append(("all negative", An, Wn, rs, cs4, torch.quantile(Dn, 0.9, dim=1).float()))
    D4, _ = _ref64(A, W, rs, cs4)
    out.append(("cscale over 4 decades", A, W, rs, cs4, torch.quantile(D4, 0.99, dim=1).float()))
    th99 = torch.quantile(D, 0.99, dim=1).float()
    for what, val in (("a zero", 0.0), ("a negative", -0.75), ("+inf", float("inf")), ("a NaN", float("nan"))):
        c = cs.clone()
        c[[3, 500, 997]] = val
        out.append((f"cscale with {what}", A, W, rs, c, th99))
    r2 = rs.clone()
    r2[::5] *= -1.0
    out.append(("negative rscale", A, W, r2, cs, th99))
    r3 = rs.clone()
    r3[::7] = float("inf")
    out.append(("infinite rscale", A, W, r3, cs, th99))
    for what, val in (("-inf", float("-inf")), ("+inf", float("inf")), ("NaN", float("nan"))):
        t = th99.clone()
        t[::2] = val
        out.append((f"theta {what}", A, W, rs, cs, t))
    return out


@pytest.mark.parametrize("cfg", G2_CFGS)
@pytest.mark.parametrize("name", ["FILTER", "FILTER_MASK", "RANK"])
def test_skip_test_changes_nothing(name, cfg):
    """with cbound = clm_value_bounds(cscale) the result is the one without it -- the same sets, the
    same cand_s bits -- and both are what S decides: thresholds most waves skip under, the cmin side
    (all scores negative), a wide cscale range, and the inputs that must switch the bound off"""
    epi = EPIS[name]
    for what, A, W, rs, cs, theta in _skip_scenarios():
        N = W.shape[0]
        allowed = torch.rand(N, generator=torch.Generator().manual_seed(11)) < 0.7
        words = _mask_words(allowed)
        margin = 0.02 if epi == RANK else 0.0
        S = _scores(cfg, A, W, rs, cs)
        keys = _bounds(cs)
        ra = Run(epi, cfg, A, W, rs, cs, theta, margin, cbound=keys, mask=words)
        ta, ba = check_bitwise(ra, S, theta, margin, allowed)
        rb = Run(epi, cfg, A, W, rs, cs, theta, margin, cbound=None, mask=words)
        tb, bb = check_bitwise(rb, S, theta, margin, allowed)
        assert _same(ra, ta, ba, rb, tb, bb), what
        if what in ("all negative", "cscale over 4 decades"):
            assert (ra.cnt[:ra.M] + ra.above[:ra.M] > 0).all(), what   # the case must have something to lose
        if what == "theta -inf" and epi == FILTER:
            assert (ra.cnt[:ra.M:2] == N).all()


@pytest.mark.parametrize("cfg", range(13))
def test_skip_test_filter_other_tiles(cfg):
    """FILTER's skip test on every tile that has it, on the two scenarios with the most to lose"""
    for what, A, W, rs, cs, theta in _skip_scenarios()[:3]:
        S = _scores(cfg, A, W, rs, cs)
        ra = Run(FILTER, cfg, A, W, rs, cs, theta, cbound=_bounds(cs))
        ta, ba = check_bitwise(ra, S, theta)
        rb = Run(FILTER, cfg, A, W, rs, cs, theta)
        tb, bb = check_bitwise(rb, S, theta)
        assert _same(ra, ta, ba, rb, tb, bb), what


@pytest.mark.parametrize("N", [1000, 1003])
@pytest.mark.parametrize("cfg", G2_CFGS)
def test_nan_scores(cfg, N):
    """NaN scores (a NaN cscale): FILTER / FILTER_MASK do not list them, RANK neither counts nor lists
    them, LSE keeps them out of the band and makes exactly their slots' partials NaN"""
    M = 70
    A, W, rs, cs, D, E, theta, allowed, words = _case(M, N, 64)
    cs = cs.clone()
    bad = [5, 130, 700]   # wave-column extents 0 / 2 / 10 at w = 64, 0 / 1 / 7 at 96, 0 / 1 / 5 at 128
    cs[bad] = float("nan")
    S = _scores(cfg, A, W, rs, cs)
    assert S[:, bad].isnan().all() and S.isnan().sum() == M * len(bad)
    ones = torch.ones(N, dtype=torch.bool)
    for epi in (FILTER, MASK, RANK, LSE):
        margin = MARGIN if epi in (RANK, LSE) else 0.0
        r = Run(epi, cfg, A, W, rs, cs, theta, margin, mask=_mask_words(ones))
        times, _ = check_bitwise(r, S, theta, margin, ones)
        assert (times[:, bad] == 0).all()
        if epi == LSE:
            _, bn, wn = TILE[cfg]
            w = bn // wn
            nslots = -(-N // bn) * wn
            nan_slots = sorted({b // w for b in bad})
            slab = r.slab[:M, :nslots]
            assert slab[:, nan_slots].isnan().all()
            rest = [j for j in range(nslots) if j not in nan_slots]
            assert slab[:, rest].isfinite().all()
            assert (r.slab[M:] == S_SENT).all() and (r.slab[:M, nslots:] == S_SENT).all()


@pytest.mark.parametrize("N", [1000, 1003])
@pytest.mark.parametrize("cfg", G2_CFGS)
def test_mask(cfg, N):
    """all ones = FILTER; all zeros = nothing; single bits at the nibble and word edges; whole clear
    stretches of 64 / 128 / 256 columns (the wave's early return); a random half; and the clear bit of
    a column far above theta never shows"""
    M, K = 70, 64
    A, W, rs, cs, D, E, _, rnd, _ = _case(M, N, K)
    theta = torch.quantile(D, 0.9, dim=1).float()
    S = _scores(cfg, A, W, rs, cs)
    rf = Run(FILTER, cfg, A, W, rs, cs, theta)
    tf, bf = check_bitwise(rf, S, theta)
    ones = torch.ones(N, dtype=torch.bool)
    r1 = Run(MASK, cfg, A, W, rs, cs, theta, mask=_mask_words(ones))
    t1, b1 = check_bitwise(r1, S, theta, allowed=ones)
    assert _same(rf, tf, bf, r1, t1, b1)
    r0 = Run(MASK, cfg, A, W, rs, cs, theta, mask=_mask_words(~ones))
    assert r0.untouched()
    low = torch.full((M,), -1e30, device="cuda")   # everything passes: the list is the mask itself
    for n in (0, 3, 4, 31, 32, N - 1):
        one = torch.zeros(N, dtype=torch.bool)
        one[n] = True
        r = Run(MASK, cfg, A, W, rs, cs, low, mask=_mask_words(one))
        times, _ = check_bitwise(r, S, low, allowed=one)
        assert (r.cnt[:M] == 1).all() and (times[:, n] == 1).all()
    holes = torch.ones(N, dtype=torch.bool)
    for a, b in ((0, 64), (128, 256), (512, 768), (960, N)):
        holes[a:b] = False
    for allowed, th in ((holes, low), (holes, theta), (rnd.cpu(), low), (rnd.cpu(), theta)):
        r = Run(MASK, cfg, A, W, rs, cs, th, mask=_mask_words(allowed), cbound=_bounds(cs))
        check_bitwise(r, S, th, allowed=allowed)
    # bits at or past N of the last word are not read: all of them set changes nothing
    words = _mask_words(rnd.cpu())
    dirty = words.clone()
    dirty[-1] |= -1 << (N % 32)   # N % 32 = 8 / 11 here: the word's upper 24 / 21 bits
    assert not torch.equal(dirty, words)
    ra = Run(MASK, cfg, A, W, rs, cs, theta, mask=words, cbound=_bounds(cs))
    ta, ba = check_bitwise(ra, S, theta, allowed=rnd)
    rb = Run(MASK, cfg, A, W, rs, cs, theta, mask=dirty, cbound=_bounds(cs))
    tb, bb = check_bitwise(rb, S, theta, allowed=rnd)
    assert _same(ra, ta, ba, rb, tb, bb)
    # columns far above theta whose bit is clear
    W2 = W.clone()
    hot = [1, 33, 254, 640, N - 2]
    W2[hot] = (A[0] * 4).half()
    S2 = _scores(cfg, A, W2, rs, cs)
    assert (S2[0, hot] > 10 * theta[0].abs() + 10).all()
    allowed = torch.ones(N, dtype=torch.bool)
    allowed[hot] = False
    r = Run(MASK, cfg, A, W2, rs, cs, theta, mask=_mask_words(allowed))
    times, _ = check_bitwise(r, S2, theta, allowed=allowed)
    assert (times[:, hot] == 0).all()


@pytest.mark.parametrize("name", list(EPIS))
def test_reproducible(name):
    """two runs: equal sets, counts, `above` and slab bits (the append order is free, nothing else)"""
    epi = EPIS[name]
    for N in (1000, 1003):
        for cfg in G2_CFGS:
            ra, ta, ba = _run_checked(epi, cfg, 300, N, 192, cbound=True)
            rb, tb, bb = _run_checked(epi, cfg, 300, N, 192, cbound=True)
            assert _same(ra, ta, ba, rb, tb, bb)


def test_empty_shapes_and_arguments():
    """M == 0 or N == 0 is CLM_OK and writes nothing; the refusals that need live device buffers"""
    A, W, rs, cs, D, E, theta, allowed, words = _case(70, 1000, 64)
    L = C.lib()
    r = Run(FILTER, 9, A[:0], W, rs, cs, theta)
    assert r.untouched()
    for epi in EPIS.values():
        r = Run(epi, 9, A, W, rs, cs, theta, MARGIN, cap=0, mask=words, expect=C.CLM_E_ARG)
        assert r.untouched()
    keys = torch.zeros(2, dtype=torch.int32, device="cuda")
    assert L.clm_value_bounds(0, C.ptr(cs), -1, C.ptr(keys), _st()) == C.CLM_E_ARG
    assert L.clm_value_bounds(0, None, 4, C.ptr(keys), _st()) == C.CLM_E_ARG
    assert L.clm_value_bounds(0, C.ptr(cs), 4, None, _st()) == C.CLM_E_ARG


# ------------------------------------------------------------------------------ value_bounds -----
def _key(f):
    b = np.asarray(f, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return np.where(b & 0x80000000, b ^ 0xFFFFFFFF, b | 0x80000000).astype(np.uint32)


def _unkey(k):
    k = np.uint32(k)
    b = np.uint32(k & np.uint32(0x7FFFFFFF)) if k & np.uint32(0x80000000) else np.uint32(~k)
    return np.array([b], dtype=np.uint32).view(np.float32)[0]


@pytest.mark.parametrize("n", [1, 255, 256, 100_003])
def test_value_bounds(n):
    """keys = float_key of numpy's min / max: positive, negative, mixed, -0.0 beside +0.0 (the key
    order puts -0.0 below +0.0), infinities; a NaN at the first, a middle or the last position makes a
    decoded bound NaN"""
    rng = np.random.default_rng(n)
    base = rng.standard_normal(n).astype(np.float32)
    cases = {"mixed": base, "positive": np.abs(base) + 0.5, "negative": -np.abs(base) - 0.5}
    z = np.abs(base)
    z[0] = 0.0
    z[n // 2] = -0.0 if n > 1 else 0.0
    cases["zeros"] = z
    inf = base.copy()
    inf[n // 3] = np.inf
    inf[-1] = -np.inf
    cases["inf"] = inf
    for what, v in cases.items():
        keys = _bounds(torch.from_numpy(v).cuda()).cpu().numpy().view(np.uint32)
        k = _key(v)
        assert keys[0] == k.min() and keys[1] == k.max(), what
        lo, hi = _unkey(keys[0]), _unkey(keys[1])
        assert lo == v.min() and hi == v.max(), what
        if what not in ("zeros",) or n == 1:
            assert keys[0] == _key(v.min()) and keys[1] == _key(v.max()), what
    for pos in sorted({0, n // 2, n - 1}):
        for nan in (np.float32(np.nan), -np.float32(np.nan)):
            v = np.abs(base) + 0.5
            v[pos] = nan
            keys = _bounds(torch.from_numpy(v).cuda()).cpu().numpy().view(np.uint32)
            assert np.isnan(_unkey(keys[0])) or np.isnan(_unkey(keys[1])), (pos, nan)
            k = _key(v)
            assert keys[0] == k.min() and keys[1] == k.max()
    empty = torch.zeros(2, dtype=torch.int32, device="cuda")
    C.check(C.lib().clm_value_bounds(0, None, 0, C.ptr(empty), _st()))
    assert empty.cpu().numpy().view(np.uint32).tolist() == [0xFFFFFFFF, 0]
