"""The encoder's row ops (k_ops.hip: the text-embedding LayerNorm, the dual in-place LayerNorm, patchify,
write_cls, gather_pooled, pool_project) and the GEMM forms only the towers run (a device-resident row
count, gemm_splitk_resid, EPI_PATCH, the unmerged-LoRA down-projection written in place), each through
its own C-ABI hook against a plain torch fp64 reference of the same operation.

Kernels that take a compute dtype run in both; write_cls, gather_pooled and pool_project are fp32 (or
plain 16-bit copies) and take none.

Every output buffer is filled with a sentinel first and is larger than what is written (extra rows, a
row stride past the width); the sentinel must survive everywhere outside the stated region.

Bars that did not exist before this file (inputs are drawn on the CPU from fixed seeds, so the figures
below are reproducible without a device):

  * fp32 `hf` of the dual LayerNorm: 4 x the largest |torch fp32 CPU layer_norm - fp64| on the same
    input, floor 1e-6. That torch error is 9.1e-07 / 1.2e-06 / 1.3e-06 / 1.4e-06 / 1.7e-06 at d = 128 /
    256 / 512 / 768 / 1024 (outputs up to 7 .. 12 in magnitude), so the bar is 3.7e-06 .. 6.7e-06.
  * pool_project: 4 x the largest |torch fp32 CPU chain - fp64 chain| (LayerNorm -> projection ->
    optional L2 norm) on the same input. That torch error, un-normalised / normalised, is
    1.6e-06 / 1.3e-07 at (d, D) = (128, 40), 3.1e-06 / 2.2e-07 at (256, 64), 2.8e-06 / 1.5e-07 at
    (768, 200) and 2.5e-06 / 6.7e-08 at (1024, 768) (un-normalised outputs up to 4.5 .. 5.9).
The tests compute the torch fp32 error themselves, on the CPU of the machine they run on.
"""
import functools

import pytest
import torch

from clip_lora_match_amd import _capi as C
from test_gpu_kernels import _g4_ok

pytestmark = pytest.mark.gpu
DT = {"bfloat16": (torch.bfloat16, C.CLM_BF16, 2.0 ** -8), "float16": (torch.float16, C.CLM_F16, 2.0 ** -11)}
DTYPES = ["bfloat16", "float16"]
WIDTHS = [128, 256, 512, 768, 1024]
SENT = -99.0
STORE_TOL = {"bfloat16": 2e-2, "float16": 4e-3}   # test_gemm_epilogues_vs_torch's 16-bit bars (x max |ref|)


def _p(t):
    return C.ptr(t) if t is not None else None


def _st():
    return C.stream_of(torch.device("cuda:0"))


def _cpu_randn(seed, *shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _sentinel(shape, dtype=torch.float32):
    return torch.full(shape, SENT, device="cuda").to(dtype)


def _ln_ex(dtype, mode, M, d, g1, b1, y, src=None, ids=None, tok=None, pos=None, L=0, hf=None, g2=None, b2=None,
           m_dev=None, rowmap=None, ldy=None):
    """clm_layernorm_ex -> return code"""
    return C.lib().clm_layernorm_ex(0, DT[dtype][1], mode, _p(src), src.stride(0) if src is not None else 0, _p(ids),
                                    _p(tok), _p(pos), L, _p(hf), hf.stride(0) if hf is not None else 0, _p(g1), _p(b1),
                                    _p(g2), _p(b2), 1e-5, _p(y), y.stride(0) if ldy is None else ldy, M, d, _p(m_dev),
                                    _p(rowmap), _st())


def _ln64(x, g, b):
    return torch.nn.functional.layer_norm(x.double(), (x.shape[-1],), g.double(), b.double(), 1e-5)


def _ln_bar_ok(dtype, y, ref):
    """the project's LayerNorm bar: one ulp of the type, relative, + 1e-6"""
    err = (y.double() - ref).abs()
    return bool((err <= DT[dtype][2] * ref.abs() + 1e-6).all()), float(err.max())


# ------------------------------------------------------------------ text embedding LN (mode 1) ---
TXT_L, TXT_B, TXT_V, TXT_EOS = 13, 5, 37, 36
TXT_LENS = (1, 13, 4, 7, 6)   # live rows per caption: 1 and L among them, odd total (31)


@functools.lru_cache(maxsize=None)
def _text_inputs(d):
    """ids [B, L] over a vocabulary of 37 (0 and 36 both present; 36 is the EOS, first at lens[b] - 1),
    token and position tables, gamma / beta"""
    g = torch.Generator().manual_seed(1000 + d)
    ids = torch.randint(1, TXT_EOS, (TXT_B, TXT_L), generator=g, dtype=torch.int32)
    ids[1, 0] = 0
    for b, n in enumerate(TXT_LENS):
        ids[b, n - 1] = TXT_EOS
    tok, pos = _cpu_randn(d, TXT_V, d), _cpu_randn(d + 1, TXT_L, d) * 0.5
    gam, bet = _cpu_randn(d + 2, d), _cpu_randn(d + 3, d)
    return tuple(t.cuda() for t in (ids, tok, pos, gam, bet))


def _text_plan(ids):
    B, L = ids.shape
    lens, offs, rowmap, tiles, counts = (torch.full((n,), -7, dtype=torch.int32, device="cuda")
                                         for n in (B, B + 1, B * L, B, 2))
    C.check(C.lib().clm_text_plan(0, C.ptr(ids), B, L, TXT_EOS, C.ptr(lens), C.ptr(offs), C.ptr(rowmap),
                                  C.ptr(tiles), C.ptr(counts), _st()), "clm_text_plan")
    return rowmap, counts, offs


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", WIDTHS)
def test_text_embedding_layernorm(dtype, d):
    """LnArgs::mode == 1 at every compiled width. (a) padded, M = B L: hf is the single rounded fp32 add
    tok[id] + pos[r % L], bit for bit, and y is the fp64 LayerNorm of it at the LayerNorm bar. (b) packed
    (rowmap, m_dev from clm_text_plan; lens 1, 13, 4, 7, 6): packed row r carries the bits of padded row
    rowmap[r] in hf and y for ldy = d, d + 4, d + 8; rows at or past *m_dev keep the sentinel. (c) *m_dev
    = 0 writes nothing."""
    td = DT[dtype][0]
    ids, tok, pos, gam, bet = _text_inputs(d)
    M = TXT_B * TXT_L
    hf = _sentinel((M + 3, d + 4))
    y = _sentinel((M + 3, d + 8), td)
    C.check(_ln_ex(dtype, 1, M, d, gam, bet, y, ids=ids, tok=tok, pos=pos, L=TXT_L, hf=hf), "clm_layernorm_ex")
    flat = ids.flatten().long()
    want_h = tok[flat] + pos[torch.arange(M, device="cuda") % TXT_L]
    assert torch.equal(hf[:M, :d], want_h)
    assert (hf[M:] == SENT).all() and (hf[:, d:] == SENT).all()
    assert (y[M:].float() == SENT).all() and (y[:, d:].float() == SENT).all()
    ok, err = _ln_bar_ok(dtype, y[:M, :d], _ln64(want_h, gam, bet))
    print(f"mode 1 {dtype} d {d}: max |y - ln64| {err:.3e}")
    assert ok, err

    rowmap, counts, _ = _text_plan(ids)
    total = int(counts[0])
    assert total == sum(TXT_LENS) and total % 2 == 1
    rm = rowmap[:total].long()
    for ldy in (d, d + 4, d + 8):
        hp = _sentinel((M + 3, d + 4))
        yp = _sentinel((M + 3, ldy), td)
        C.check(_ln_ex(dtype, 1, M, d, gam, bet, yp, ids=ids, tok=tok, pos=pos, L=TXT_L, hf=hp, m_dev=counts,
                       rowmap=rowmap), "clm_layernorm_ex")
        assert torch.equal(hp[:total, :d], hf[rm, :d]), ldy
        assert torch.equal(yp[:total, :d], y[rm, :d]), ldy
        assert (hp[total:] == SENT).all() and (hp[:, d:] == SENT).all(), ldy
        assert (yp[total:].float() == SENT).all() and (yp[:, d:].float() == SENT).all(), ldy

    zero = torch.zeros(2, dtype=torch.int32, device="cuda")
    hz, yz = _sentinel((M + 3, d + 4)), _sentinel((M + 3, d + 8), td)
    C.check(_ln_ex(dtype, 1, M, d, gam, bet, yz, ids=ids, tok=tok, pos=pos, L=TXT_L, hf=hz, m_dev=zero,
                   rowmap=rowmap), "clm_layernorm_ex")
    assert (hz == SENT).all() and (yz.float() == SENT).all()


def test_layernorm_ex_refusals_write_nothing():
    """what clm_layernorm refuses, and mode 1 without ids / tok / pos / hf or with L < 1, a lone g2, a
    rowmap in mode 0: CLM_E_ARG, nothing written"""
    d, M = 256, 8
    ids, tok, pos, gam, bet = _text_inputs(d)
    hf, y = _sentinel((M, d)), _sentinel((M, d), torch.float16)
    src = torch.zeros((M, d), device="cuda")
    full = dict(ids=ids, tok=tok, pos=pos, L=TXT_L, hf=hf)
    for drop in ("ids", "tok", "pos", "hf"):
        assert _ln_ex("float16", 1, M, d, gam, bet, y, **dict(full, **{drop: None})) == C.CLM_E_ARG, drop
    assert _ln_ex("float16", 1, M, d, gam, bet, y, **dict(full, L=0)) == C.CLM_E_ARG
    assert _ln_ex("float16", 2, M, d, gam, bet, y, src=src) == C.CLM_E_ARG
    assert _ln_ex("float16", 0, M, d, gam, bet, y, src=src, hf=hf, g2=gam) == C.CLM_E_ARG       # g2 without b2
    assert _ln_ex("float16", 0, M, d, gam, bet, y, src=src, g2=gam, b2=bet) == C.CLM_E_ARG       # g2 without hf
    assert _ln_ex("float16", 0, M, d, gam, bet, y, src=src, rowmap=ids) == C.CLM_E_ARG
    assert _ln_ex("float16", 0, M, d, gam, bet, y, src=None) == C.CLM_E_ARG
    assert _ln_ex("float16", 0, M, 100, gam, bet, y, src=src) == C.CLM_E_ARG
    assert _ln_ex("float16", 0, M, d, gam, bet, y, src=src, ldy=d - 4) == C.CLM_E_ARG
    assert _ln_ex("float16", 0, M, d, gam, bet, y, src=src, ldy=d + 2) == C.CLM_E_ARG
    assert _ln_ex("float16", 0, -1, d, gam, bet, y, src=src) == C.CLM_E_ARG
    assert C.lib().clm_layernorm_ex(0, C.CLM_F32, 0, C.ptr(src), d, None, None, None, 0, None, 0, C.ptr(gam),
                                    C.ptr(bet), None, None, 1e-5, C.ptr(y), d, M, d, None, None, _st()) == C.CLM_E_ARG
    assert _ln_ex("float16", 0, 0, d, gam, bet, y, src=src) == C.CLM_OK
    torch.cuda.synchronize()
    assert (hf == SENT).all() and (y.float() == SENT).all()


# ------------------------------------------------------------------ dual LN, in place ---
@functools.lru_cache(maxsize=None)
def _dual_inputs(d):
    """x [50, d] (rows with a common offset, as a residual stream has), two gamma / beta pairs, the fp64
    LN1, and torch's fp32 CPU layer_norm error against it -- all on the CPU"""
    x = _cpu_randn(2000 + d, 50, d) * 3 + _cpu_randn(2001 + d, 50, 1) * 5
    g1, b1, g2, b2 = (_cpu_randn(2002 + d + i, d) for i in range(4))
    ref1 = _ln64(x, g1, b1)
    e32 = float((torch.nn.functional.layer_norm(x, (d,), g1, b1, 1e-5).double() - ref1).abs().max())
    return x.cuda(), g1.cuda(), b1.cuda(), g2.cuda(), b2.cuda(), ref1.cuda(), e32


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", WIDTHS)
def test_dual_layernorm_in_place(dtype, d):
    """g2 != null with src == hf (image_prologue's pre-LN + layer-0 LN1), M = 50, 1, 2, 7, 9. hf against
    the fp64 LN1: bar 4 x torch's own fp32 CPU layer_norm error on this input (9e-07 .. 1.7e-06, see the
    module docstring), floor 1e-6. y against the fp64 LN2 of the stored hf at the LayerNorm bar. A row's
    bits (hf and y) do not depend on M, nor on whether M or a device-resident *m_dev gives the row count
    (rows at or past *m_dev keep their source values and the sentinel)."""
    td = DT[dtype][0]
    x, g1, b1, g2, b2, ref1, e32 = _dual_inputs(d)
    bar = max(4 * e32, 1e-6)
    first = None
    for M in (50, 1, 2, 7, 9):
        h = _sentinel((M + 3, d + 4))
        h[:M, :d] = x[:M]
        y = _sentinel((M + 3, d + 8), td)
        C.check(_ln_ex(dtype, 0, M, d, g1, b1, y, src=h, hf=h, g2=g2, b2=b2), "clm_layernorm_ex")
        assert (h[M:] == SENT).all() and (h[:, d:] == SENT).all(), M
        assert (y[M:].float() == SENT).all() and (y[:, d:].float() == SENT).all(), M
        eh = float((h[:M, :d].double() - ref1[:M]).abs().max())
        ok, ey = _ln_bar_ok(dtype, y[:M, :d], _ln64(h[:M, :d], g2, b2))
        print(f"dual LN {dtype} d {d} M {M}: max |hf - ln64| {eh:.3e} (torch fp32 {e32:.3e}, bar {bar:.3e}), "
              f"max |y - ln64(hf)| {ey:.3e}")
        assert eh <= bar, (M, eh, bar)
        assert ok, (M, ey)
        if first is None:
            first = (h[:M, :d].clone(), y[:M, :d].clone())
        assert torch.equal(h[:M, :d], first[0][:M]) and torch.equal(y[:M, :d], first[1][:M]), M
    # the device-resident row count in mode 0: M = 50 sizes the grid, *m_dev = 9 rows are normalised
    mdev = torch.tensor([9, 50], dtype=torch.int32, device="cuda")
    h = _sentinel((53, d + 4))
    h[:50, :d] = x
    y = _sentinel((53, d + 8), td)
    C.check(_ln_ex(dtype, 0, 50, d, g1, b1, y, src=h, hf=h, g2=g2, b2=b2, m_dev=mdev), "clm_layernorm_ex")
    assert torch.equal(h[:9, :d], first[0][:9]) and torch.equal(y[:9, :d], first[1][:9])
    assert torch.equal(h[9:50, :d], x[9:]) and (h[50:] == SENT).all() and (h[:, d:] == SENT).all()
    assert (y[9:].float() == SENT).all() and (y[:, d:].float() == SENT).all()


# ------------------------------------------------------------------ patchify ---
def _patchify(dtype, pix, layout, B, S, p, Cn, lut, P, Kp):
    return C.lib().clm_patchify(0, DT[dtype][1], C.ptr(pix), layout, B, S, p, Cn, _p(lut), C.ptr(P), Kp, _st())


def _patch_case(dtype, layout, B, S, p, Cn, Kp, seed):
    """one patchify call into a sentinel buffer with 3 spare rows -> (P, the unfold reference rounded
    once to the compute dtype [B G G, C p p])"""
    td = DT[dtype][0]
    g = torch.Generator().manual_seed(seed)
    lut = torch.randn((Cn, 256), generator=g).cuda()
    if layout == C.CLM_PIX_U8_HWC:
        pix = torch.randint(0, 256, (B, S, S, Cn), generator=g, dtype=torch.uint8).cuda()
        img = torch.stack([lut[c][pix[..., c].long()] for c in range(Cn)], 1)     # [B, C, S, S]
    else:
        pix = torch.randn((B, Cn, S, S), generator=g).cuda()
        img = pix
    G = S // p
    ref = torch.nn.functional.unfold(img, kernel_size=p, stride=p).transpose(1, 2).reshape(B * G * G, Cn * p * p)
    P = _sentinel((B * G * G + 3, Kp), td)
    rc = _patchify(dtype, pix, layout, B, S, p, Cn, lut, P, Kp)
    return rc, P, ref.to(td)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", [C.CLM_PIX_U8_HWC, C.CLM_PIX_F32_CHW])
def test_patchify_exact(dtype, layout):
    """(S, p) = (16, 8) and (32, 16) on the fast path, (28, 14) on the generic one, C = 3, B = 1 and 3,
    Kp = 3 p^2 rounded up to 64 and 64 more (the fast path's pad_cols_kernel), and C = 1 on the generic
    path: the values are LUT entries or copies rounded once, so equality is exact; padding columns are
    exactly zero; rows past B G^2 keep the sentinel. Kp % 8 != 0 is refused with nothing written."""
    cases = [(S, p, 3, B, k0 + extra) for S, p, k0 in ((16, 8, 192), (32, 16, 768), (28, 14, 640))
             for B in (1, 3) for extra in (0, 64)] + [(28, 14, 1, 2, 256)]
    for i, (S, p, Cn, B, Kp) in enumerate(cases):
        rc, P, ref = _patch_case(dtype, layout, B, S, p, Cn, Kp, 3000 + i)
        C.check(rc, "clm_patchify")
        rows, kreal = ref.shape
        assert torch.equal(P[:rows, :kreal], ref), (S, p, Cn, B, Kp)
        assert (P[:rows, kreal:].float() == 0).all(), (S, p, Cn, B, Kp)
        assert (P[rows:].float() == SENT).all(), (S, p, Cn, B, Kp)
    for S, p, Cn, Kp in ((28, 14, 1, 196), (16, 8, 3, 196)):
        rc, P, _ = _patch_case(dtype, layout, 2, S, p, Cn, Kp, 3100)
        torch.cuda.synchronize()
        assert rc != C.CLM_OK and (P.float() == SENT).all(), (S, p, Cn, Kp)
    rc, P, _ = _patch_case(dtype, layout, 2, 16, 8, 3, 128, 3101)   # Kp < C p^2: the hook's own check
    assert rc == C.CLM_E_ARG and (P.float() == SENT).all()


# ------------------------------------------------------------------ write_cls, gather_pooled ---
def test_write_cls_exact():
    """h[b T, :d] = cls + pos[0] (one fp32 add) with ldh > d; every other row and column untouched"""
    B, T, d, ldh = 3, 5, 300, 304
    cls, pos = _cpu_randn(40, d).cuda(), _cpu_randn(41, T, d).cuda()
    h = _sentinel((B * T + 2, ldh))
    C.check(C.lib().clm_write_cls(0, C.ptr(h), ldh, B, T, d, C.ptr(cls), C.ptr(pos), _st()), "clm_write_cls")
    want = _sentinel((B * T + 2, ldh))
    want[0:B * T:T, :d] = cls + pos[0]
    assert torch.equal(h, want)
    assert C.lib().clm_write_cls(0, C.ptr(h), d - 4, B, T, d, C.ptr(cls), C.ptr(pos), _st()) == C.CLM_E_ARG
    assert C.lib().clm_write_cls(0, C.ptr(h), ldh, B, T, d, None, C.ptr(pos), _st()) == C.CLM_E_ARG


POOL_T = 77


def _pool_ids(eos):
    """captions [6, 77] and their pooled rows: EOS positions past lane 63, repeated EOS / maxima (the first
    counts), and one caption without an EOS (first-match rule: row 0)"""
    g = torch.Generator().manual_seed(50 + eos)
    if eos == 2:   # the legacy rule: argmax, first of the maxima
        ids = torch.randint(3, 900, (6, POOL_T), generator=g, dtype=torch.int32)
        rows = [70, 64, 0, 76, 3, 65]
        for b, r in enumerate(rows):
            ids[b, r] = 1000 + b
        ids[0, 75] = 1000      # a tie later in the caption
        ids[4, 70] = 1004
        ids[5, 1] = 1005 - 1   # a near-maximum earlier
    else:
        ids = torch.randint(0, eos, (6, POOL_T), generator=g, dtype=torch.int32)
        rows = [70, 64, 0, 76, 3, 0]
        for b, r in enumerate(rows[:5]):   # caption 5 has none: row 0
            ids[b, r] = eos
        ids[0, 75] = eos       # later repeats
        ids[4, 70] = eos
        ids[2, 5] = eos
    return ids.cuda(), rows


def _pool_modes():
    """(name, T, ids, eos, offs, pooled row of item b in h) for 17 items"""
    out = []
    for eos in (2, 36):
        ids6, rows6 = _pool_ids(eos)
        ids = torch.cat([ids6, ids6, ids6])[:17].contiguous()
        rows = (rows6 * 3)[:17]
        out.append((f"eos{eos}", POOL_T, ids, eos, None, [b * POOL_T + r for b, r in enumerate(rows)]))
    out.append(("cls", 3, None, 36, None, [b * 3 for b in range(17)]))
    lens = [1, 13, 4, 7, 6, 2, 9, 1, 3, 5, 8, 2, 2, 11, 1, 6, 4]
    offs = torch.tensor([sum(lens[:b]) for b in range(18)], dtype=torch.int32)
    out.append(("offs", POOL_T, None, 36, offs.cuda(), [int(offs[b + 1]) - 1 for b in range(17)]))
    return {m[0]: m for m in out}


@pytest.mark.parametrize("mode", ["eos2", "eos36", "cls", "offs"])
def test_gather_pooled_exact(mode):
    """hc[b] = h[pooled row][:d], Oc[b][:d] = O[pooled row][:d], copies, with ldh > d and ldoc != ldo;
    the pooled row under both EOS rules (T = 77), with ids == null (row b T) and with offs; Oc's columns
    past d and every row past B untouched"""
    _, T, ids, eos, offs, prow = _pool_modes()[mode]
    B, d = 6, 264
    nrows = max(prow[:B]) + 1 if mode == "offs" else B * T
    h = _cpu_randn(60, nrows, d + 4).cuda()
    O = torch.randint(-30000, 30000, (nrows, d + 8), generator=torch.Generator().manual_seed(61),
                      dtype=torch.int16).cuda()
    hc = _sentinel((B + 2, d))
    Oc = torch.full((B + 2, d + 16), -99, dtype=torch.int16, device="cuda")
    C.check(C.lib().clm_gather_pooled(0, C.ptr(h), h.stride(0), C.ptr(O), O.stride(0), B, T, d, _p(ids), eos,
                                      C.ptr(hc), C.ptr(Oc), Oc.stride(0), _p(offs), _st()), "clm_gather_pooled")
    idx = torch.tensor(prow[:B], device="cuda")
    assert torch.equal(hc[:B], h[idx, :d]) and (hc[B:] == SENT).all()
    assert torch.equal(Oc[:B, :d], O[idx, :d]) and (Oc[B:] == -99).all() and (Oc[:, d:] == -99).all()
    rc = C.lib().clm_gather_pooled(0, C.ptr(h), h.stride(0), C.ptr(O), O.stride(0), B, T, d, _p(ids), eos,
                                   C.ptr(hc), C.ptr(Oc), d + 2, _p(offs), _st())   # ldoc % 4 != 0: the launcher's
    assert rc == C.CLM_E_HIP
    rc = C.lib().clm_gather_pooled(0, C.ptr(h), d - 4, C.ptr(O), O.stride(0), B, T, d, _p(ids), eos, C.ptr(hc),
                                   C.ptr(Oc), Oc.stride(0), _p(offs), _st())
    assert rc == C.CLM_E_ARG


# ------------------------------------------------------------------ pool_project ---
def _pool_project(h, B, T, d, ids, eos, gam, bet, projT, D, tmp, out, normalize, offs):
    odt = C.CLM_F32 if out.dtype == torch.float32 else C.CLM_F16
    return C.lib().clm_pool_project(0, C.ptr(h), h.stride(0), B, T, d, _p(ids), eos, C.ptr(gam), C.ptr(bet), 1e-5,
                                    C.ptr(projT), D, C.ptr(tmp), C.ptr(out), odt, normalize, _p(offs), _st())


@functools.lru_cache(maxsize=None)
def _pool_inputs(d, D):
    """pooled rows x [17, d], gamma / beta, projT [d, D] on the CPU, the fp64 chain (un-normalised and
    normalised) and torch's fp32 CPU error against it"""
    x = _cpu_randn(70 + d, 17, d) * 2 + _cpu_randn(71 + d, 17, 1)
    gam, bet = _cpu_randn(72 + d, d), _cpu_randn(73 + d, d)
    projT = _cpu_randn(74 + d, d, D) / d ** 0.5
    r64 = _ln64(x, gam, bet) @ projT.double()
    n64 = r64 / r64.norm(dim=1, keepdim=True)
    r32 = torch.nn.functional.layer_norm(x, (d,), gam, bet, 1e-5) @ projT
    n32 = r32 / r32.norm(dim=1, keepdim=True)
    e32 = (float((r32.double() - r64).abs().max()), float((n32.double() - n64).abs().max()))
    return x, gam.cuda(), bet.cuda(), projT.cuda(), (r64.cuda(), n64.cuda()), e32


@pytest.mark.parametrize("mode", ["eos2", "eos36", "cls", "offs"])
@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("d,D", [(128, 40), (256, 64), (768, 200), (1024, 768)])
def test_pool_project(d, D, normalize, mode):
    """pooled row -> LayerNorm -> projection -> optional L2 norm, D % 64 != 0 among the shapes, all pooling
    modes. (a) against the fp64 chain: bar 4 x the error of the same chain in torch fp32 on the CPU (see the
    module docstring for the figures). (b) for B = 1, 7, 8, 9, 17 row b carries the bits of a call that holds
    item b alone. (c) the f16 output is .half() of the f32 output, bit for bit. (d) tmp and out are
    untouched past B rows."""
    x, gam, bet, projT, refs, e32 = _pool_inputs(d, D)
    _, T, ids, eos, offs, prow = _pool_modes()[mode]
    nrows = max(prow) + 1 if mode == "offs" else 17 * T
    h = _cpu_randn(80 + d, nrows, d + 4).cuda()
    h[torch.tensor(prow, device="cuda"), :d] = x.cuda()
    ref, bar = refs[normalize], 4 * e32[normalize]

    def run(B, b0=0, odt=torch.float32):
        """items [b0, b0 + B) as one call"""
        tmp, out = _sentinel((B + 2, D)), _sentinel((B + 2, D), odt)
        hv = h if mode == "offs" else h[b0 * T:]
        C.check(_pool_project(hv, B, T, d, ids[b0:] if ids is not None else None, eos, gam, bet, projT, D, tmp, out,
                              normalize, offs[b0:] if offs is not None else None), "clm_pool_project")
        assert (tmp[B:] == SENT).all() and (out[B:].float() == SENT).all(), (B, b0)
        return out[:B]

    full = run(17)
    err = float((full.double() - ref).abs().max())
    print(f"pool_project d {d} D {D} normalize {normalize} {mode}: max |out - ref64| {err:.3e} "
          f"(torch fp32 {e32[normalize]:.3e}, bar {bar:.3e})")
    assert err <= bar, (err, bar)
    single = torch.cat([run(1, b) for b in range(17)])
    for B in (1, 7, 8, 9, 17):
        assert torch.equal(run(B), single[:B]), B
    assert torch.equal(run(17, odt=torch.float16), full.half())
    assert torch.equal(run(9, 8), single[8:17])   # a sub-batch that starts inside the second 8-row group


def test_pool_project_refusals():
    x, gam, bet, projT, _, _ = _pool_inputs(128, 40)
    h = torch.zeros((4, 128), device="cuda")
    tmp, out = _sentinel((4, 40)), _sentinel((4, 40))
    lib = C.lib()

    def call(ldh=128, B=2, d=128, odt=C.CLM_F32, g=gam, o=out):
        return lib.clm_pool_project(0, C.ptr(h), ldh, B, 1, d, None, 2, _p(g), C.ptr(bet), 1e-5, C.ptr(projT), 40,
                                    C.ptr(tmp), _p(o), odt, 1, None, _st())
    assert call(odt=C.CLM_BF16) == C.CLM_E_ARG
    assert call(B=-1) == C.CLM_E_ARG
    assert call(ldh=64) == C.CLM_E_ARG
    assert call(g=None) == C.CLM_E_ARG
    assert call(o=None) == C.CLM_E_ARG
    assert call(d=2048, ldh=2048) == C.CLM_E_ARG
    assert call(d=72, ldh=128) == C.CLM_E_HIP    # d % 16 != 0: the launcher's
    assert call(B=0) == C.CLM_OK
    torch.cuda.synchronize()
    assert (tmp == SENT).all() and (out == SENT).all()


# ------------------------------------------------------------------ GEMM forms ---
def _gemm_ex(dtype, epi, cfg, A, W, M, N, K, out, ldo, bias=None, aux=None, aux_ld=0, group=0, m_dev=None, slices=0,
             ws=None, lda=None):
    """clm_gemm_ex -> return code"""
    return C.lib().clm_gemm_ex(0, DT[dtype][1], epi, cfg, C.ptr(A), A.stride(0) if lda is None else lda, C.ptr(W),
                               W.stride(0), M, N, K, C.ptr(out), ldo, _p(bias), _p(aux), aux_ld, group, _p(m_dev),
                               slices, _p(ws), _st())


def _configs(epi, N, K, ldo):
    return [c for c in list(range(C.lib().clm_gemm_num_configs())) + [-1] if _g4_ok(c, epi, N, K, ldo)]


def _operands(dtype, M, N, K, seed):
    td = DT[dtype][0]
    A = _cpu_randn(seed, M, K).cuda().to(td)
    W = (_cpu_randn(seed + 1, N, K) / K ** 0.5).cuda().to(td)
    bias = _cpu_randn(seed + 2, N).cuda()
    return A, W, bias


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("epi", ["STORE", "GELU", "RESID"])
def test_gemm_device_row_count(dtype, epi):
    """GemmArgs::m_dev in every configuration family (gemm_kernel, G2, G4) and the heuristic: with M = 200
    sizing the grid and *m_dev = 0, 1, 77, 200, rows below *m_dev carry the bits of a plain call with M =
    *m_dev; rows at or past it and the pad columns (ldo = N + 8) keep what they held; *m_dev = 0 is a clean
    no-op."""
    M, N, K = 200, 136, 192
    ldo = N + 8
    code = getattr(C, f"CLM_EPI_{epi}")
    A, W, bias = _operands(dtype, M, N, K, 90)
    if epi == "RESID":
        init = _cpu_randn(93, M + 3, ldo).cuda()
    else:
        init = _sentinel((M + 3, ldo), DT[dtype][0])
    cfgs = _configs(code, N, K, ldo)
    assert len(cfgs) == 16
    for cfg in cfgs:
        for md in (0, 1, 77, 200):
            want = init.clone()
            if md:
                C.check(_gemm_ex(dtype, code, cfg, A, W, md, N, K, want, ldo, bias), "clm_gemm_ex")
                assert torch.equal(want[md:], init[md:]) and torch.equal(want[:, N:], init[:, N:]), (cfg, md)
                assert not torch.equal(want[:md, :N], init[:md, :N])
            got = init.clone()
            mdev = torch.tensor([md, 12345], dtype=torch.int32, device="cuda")
            C.check(_gemm_ex(dtype, code, cfg, A, W, M, N, K, got, ldo, bias, m_dev=mdev), "clm_gemm_ex")
            assert torch.equal(got, want), (cfg, md)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [64, 200])
def test_gemm_splitk_resid(dtype, N):
    """gemm_splitk_resid, K = 768, slices over every divisor of 12, M = 129 (across the 128-row tile), 1, 3,
    8: out = h0 + A W^T + bias against fp64 at the RESID bar (1e-3 max |ref| + 1e-5); for a fixed slice
    count a row's bits do not depend on M and are those of the per-slice plain GEMMs summed in slice order;
    ws is untouched past slices M N floats and out's pad columns
    and spare rows are untouched. N % 4 != 0, K % (64 slices) != 0 and a null ws are refused with nothing
    written."""
    K, Mmax = 768, 129
    ldo = N + 8
    A, W, bias = _operands(dtype, Mmax, N, K, 100 + N)
    h0 = _cpu_randn(104, Mmax + 2, ldo).cuda()
    ref = A.double() @ W.double().T + bias.double()
    bar = 1e-3 * float(ref.abs().max()) + 1e-5
    for slices in (1, 2, 3, 4, 6, 12):
        first = None
        for M in (129, 1, 3, 8):
            out = h0[:M + 2].clone()
            ws = _sentinel((slices * M * N + 64,))
            C.check(_gemm_ex(dtype, C.CLM_EPI_RESID, -1, A, W, M, N, K, out, ldo, bias, slices=slices, ws=ws),
                    "clm_gemm_ex")
            assert (ws[slices * M * N:] == SENT).all(), (slices, M)
            assert torch.equal(out[M:], h0[M:M + 2]) and torch.equal(out[:, N:], h0[:M + 2, N:]), (slices, M)
            err = float((out[:M, :N].double() - (h0[:M, :N].double() + ref[:M])).abs().max())
            assert err <= bar, (slices, M, err, bar)
            if first is None:
                first = out[:M, :N].clone()
                # "summed in slice order": the bits of h0 + ((p_0 + p_1 + ...) + bias), p_s the plain fp32
                # GEMM over K slice s (clm_gemm, SCORE with no scales stores acc as it is)
                ks, acc = K // slices, None
                for s in range(slices):
                    p = torch.empty((M, N), device="cuda")
                    C.check(C.lib().clm_gemm(0, DT[dtype][1], C.CLM_EPI_SCORE, -1, C.ptr(A[:, s * ks:]), K,
                                             C.ptr(W[:, s * ks:]), K, M, N, ks, C.ptr(p), N, None, None, None, _st()),
                            "clm_gemm")
                    acc = p if acc is None else acc + p
                assert torch.equal(first, h0[:M, :N] + (acc + bias)), slices
            assert torch.equal(out[:M, :N], first[:M]), (slices, M)
    out, ws = h0[:10].clone(), _sentinel((12 * 8 * 256,))
    Wr = torch.cat([W, W])[:N + 2].contiguous()
    bad = [dict(N=N + 2, W=Wr, slices=2, ws=ws),      # N % 4 != 0
           dict(N=N, W=W, slices=5, ws=ws),           # K % (64 slices) != 0
           dict(N=N, W=W, slices=8, ws=ws),
           dict(N=N, W=W, slices=2, ws=None)]         # no workspace
    for b in bad:
        rc = _gemm_ex(dtype, C.CLM_EPI_RESID, -1, A, b["W"], 8, b["N"], K, out, ldo, bias, slices=b["slices"],
                      ws=b["ws"])
        torch.cuda.synchronize()
        assert rc != C.CLM_OK and torch.equal(out, h0[:10]) and (ws == SENT).all(), b["slices"]
    mdev = torch.tensor([4], dtype=torch.int32, device="cuda")
    assert _gemm_ex(dtype, C.CLM_EPI_RESID, -1, A, W, 8, N, K, out, ldo, bias, slices=2, ws=ws,
                    m_dev=mdev) == C.CLM_E_ARG                                     # the reduce pass takes no m_dev
    assert _gemm_ex(dtype, C.CLM_EPI_STORE, -1, A, W, 8, N, K, out, ldo, bias, slices=2, ws=ws) == C.CLM_E_ARG
    assert _gemm_ex(dtype, C.CLM_EPI_RESID, -1, A, W, 8, N, K, out, ldo, bias, slices=0, ws=ws) == C.CLM_E_ARG
    assert torch.equal(out, h0[:10]) and (ws == SENT).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [128, 50])
@pytest.mark.parametrize("group,B", [(1, 260), (5, 52), (49, 5), (130, 2)])
def test_gemm_epi_patch(dtype, N, group, B):
    """EPI_PATCH on the vector (N = 128) and scalar (N = 50) epilogue paths, in every configuration that
    has it (gemm_kernel and G2; G4 refuses): tiles straddle images (group 1, 5, 49) and one image spans two
    128-row tiles (group 130). out[b (group + 1) + 1 + p, n] against fp64 acc + aux[1 + p, n] at the RESID
    bar; the class rows b (group + 1), the pad columns and the spare rows keep the sentinel; all
    configurations agree bit for bit. The bias rule (kernels.hpp): EPI_PATCH takes no bias -- one given is
    refused by the launcher on both paths, nothing written."""
    M, K = B * group, 128
    ldo, aux_ld = N + 8 + (N % 4), N + 4
    A, W, bias = _operands(dtype, M, N, K, 110 + group)
    aux = _cpu_randn(113 + group, group + 1, aux_ld).cuda()
    acc = A.double() @ W.double().T
    bar = 1e-3 * float(acc.abs().max()) + 1e-5
    rows = B * (group + 1)
    want = (acc.view(B, group, N) + aux[1:, :N].double()).reshape(M, N)
    patch_rows = torch.arange(rows, device="cuda").view(B, group + 1)[:, 1:].reshape(-1)
    first = None
    for cfg in list(range(C.lib().clm_gemm_num_configs())) + [-1]:
        out = _sentinel((rows + 2, ldo))
        rc = _gemm_ex(dtype, C.CLM_EPI_PATCH, cfg, A, W, M, N, K, out, ldo, aux=aux, aux_ld=aux_ld, group=group)
        if cfg >= 13:
            assert rc == C.CLM_E_HIP and (out == SENT).all(), cfg
            continue
        C.check(rc, "clm_gemm_ex")
        err = float((out[patch_rows, :N].double() - want).abs().max())
        assert err <= bar, (cfg, err, bar)
        assert (out[0:rows:group + 1] == SENT).all() and (out[rows:] == SENT).all() and (out[:, N:] == SENT).all(), cfg
        if first is None:
            first = out
        assert torch.equal(out, first), cfg
    for cfg in (-1, 0, 9):
        out = _sentinel((rows + 2, ldo))
        rc = _gemm_ex(dtype, C.CLM_EPI_PATCH, cfg, A, W, M, N, K, out, ldo, bias, aux=aux, aux_ld=aux_ld, group=group)
        torch.cuda.synchronize()
        assert rc == C.CLM_E_HIP and (out == SENT).all(), cfg
    out = _sentinel((rows + 2, ldo))
    ex = dict(aux=aux, aux_ld=aux_ld, group=group)
    assert _gemm_ex(dtype, C.CLM_EPI_PATCH, -1, A, W, M, N, K, out, ldo, **dict(ex, aux=None)) == C.CLM_E_ARG
    assert _gemm_ex(dtype, C.CLM_EPI_PATCH, -1, A, W, M, N, K, out, ldo, **dict(ex, group=0)) == C.CLM_E_ARG
    assert _gemm_ex(dtype, C.CLM_EPI_PATCH, -1, A, W, M, N, K, out, ldo, **dict(ex, aux_ld=N - 2)) == C.CLM_E_ARG
    if group > 1:
        assert _gemm_ex(dtype, C.CLM_EPI_PATCH, -1, A, W, M - 1, N, K, out, ldo, **ex) == C.CLM_E_ARG
    assert _gemm_ex(dtype, C.CLM_EPI_RESID, -1, A, W, M, N, K, out, ldo, **ex) == C.CLM_E_ARG   # aux is PATCH's
    assert (out == SENT).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [128, 512])
def test_lora_down_projection_in_place(dtype, K):
    """lora_down_gemm's form: X [150, ldx = K + 64], out = X + K, ldo = ldx, N = 64 -- the output goes into
    the padding columns of its own A operand, which start as NaN. A [64, K] has rank rows r = 16 and zeros
    below. Through clm_gemm (aliased pointers), config 12 and the heuristic: X[:, :K] keeps its bits,
    X[:, K:K+64] = round16(X A^T) within the STORE bar with columns >= r exactly zero and no NaN left. The
    consumer GEMM over K_eff = K + 32 with W_ext = [W | s B | finite filler] matches fp64 x W^T + round16(x
    A^T) (s B)^T + bias at the 16-bit STORE bar. Through clm_gemm_ex with *m_dev = 77, rows at or past 77
    keep their NaN extension and the rows below carry the plain call's bits."""
    td, tol = DT[dtype][0], STORE_TOL[dtype]
    M, r, ldx, Nc, s = 150, 16, K + 64, 136, 0.5
    g = torch.Generator().manual_seed(120 + K)
    x = torch.randn((M, K), generator=g).cuda().to(td)
    Am = torch.zeros((64, K))
    Am[:r] = torch.randn((r, K), generator=g) / K ** 0.5
    Am = Am.cuda().to(td)
    Wc = (torch.randn((Nc, K), generator=g) / K ** 0.5).cuda().to(td)
    Bm = torch.randn((Nc, r), generator=g).cuda()
    bias = torch.randn(Nc, generator=g).cuda()
    Wext = torch.randn((Nc, ldx), generator=g).cuda()
    Wext[:, :K] = Wc.float()
    Wext[:, K:K + r] = s * Bm
    Wext = Wext.to(td)
    down64 = x.double() @ Am.double().T
    down16 = down64.to(td)
    ref = x.double() @ Wc.double().T + down16[:, :r].double() @ Wext[:, K:K + r].double().T + bias.double()

    def fresh():
        X = torch.full((M + 2, ldx), float("nan"), device="cuda").to(td)
        X[:M, :K] = x
        return X

    results = []
    for cfg in (12, -1):
        X = fresh()
        ext = X[:, K:]   # the view whose data pointer is X + K
        C.check(C.lib().clm_gemm(0, DT[dtype][1], C.CLM_EPI_STORE, cfg, C.ptr(X), ldx, C.ptr(Am), K, M, 64, K,
                                 C.ptr(ext), ldx, None, None, None, _st()), "clm_gemm")
        assert torch.equal(X[:M, :K], x), cfg
        assert torch.isnan(X[M:].float()).all(), cfg
        got = X[:M, K:].float()
        assert not torch.isnan(got).any(), cfg
        assert (got[:, r:] == 0).all(), cfg
        err = float((got.double() - down64).abs().max())
        assert err <= tol * float(down64.abs().max()), (cfg, err)
        out = _sentinel((M + 2, Nc + 8), td)
        C.check(C.lib().clm_gemm(0, DT[dtype][1], C.CLM_EPI_STORE, -1, C.ptr(X), ldx, C.ptr(Wext), ldx, M, Nc, K + 32,
                                 C.ptr(out), out.stride(0), C.ptr(bias), None, None, _st()), "clm_gemm")
        errc = float((out[:M, :Nc].double() - ref).abs().max())
        assert errc <= tol * float(ref.abs().max()), (cfg, errc)
        assert (out[M:].float() == SENT).all() and (out[:, Nc:].float() == SENT).all(), cfg
        results.append(X)
    assert torch.equal(results[0][:M], results[1][:M])

    mdev = torch.tensor([77], dtype=torch.int32, device="cuda")
    for cfg in (12, -1):
        X = fresh()
        C.check(_gemm_ex(dtype, C.CLM_EPI_STORE, cfg, X, Am, M, 64, K, X[:, K:], ldx, m_dev=mdev, lda=ldx),
                "clm_gemm_ex")
        assert torch.equal(X[:77], results[0][:77]), cfg
        assert torch.equal(X[77:M, :K], x[77:]) and torch.isnan(X[77:, K:].float()).all(), cfg
