"""Every attention kernel of k_attn.hip on inputs with exactly known answers (tests/attn_families.py:
one key, or two equally scored keys in different key tiles, per query; integer V rows that differ from
key to key), at the tile edges, held to half an ulp of the output type against an fp64 reference -- a
dropped, misplaced or wrongly masked key moves an answer by 0.5 or more. The kernels behind
$CLM_ATTN_LONG run in child processes. And the LayerNorm hook's remaining kernels and store paths."""
import os
import subprocess
import sys

import pytest
import torch

import attn_families as F
from conftest import REPO

from clip_lora_match_amd import _capi as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
@pytest.mark.parametrize("T", F.SMALL_T)
def test_attn_small_kernel_families(dtype, T):
    """attn_small_kernel (T <= 128; 16-query waves, two 64-key tiles): a wave exactly full or holding
    one query (15 / 16 / 17 ...), the second key tile empty, holding one key or full (64 / 65 / 128),
    the causal nkt switching from 1 to 2 tiles. Non-causal: single and pair; causal: causal_pairs."""
    errs = {f: F.run_on_gpu(f, T, f == "causal_pairs", dtype) for f in F.FAMILIES}
    print(f"attn_small_kernel {dtype} T {T}: max |out - ref64| {errs}")


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
@pytest.mark.parametrize("T", F.DMA_T)
def test_attn_long_dma_kernel_families(dtype, T):
    """attn_long_dma_kernel (T > 128 non-causal, the default): no masked tail (192, 256, 320), a tail of
    one key (129, 193, 257, 577), one query in the last 128-query block (129, 257); the pair family puts
    the two keys in different tiles, so the answer depends on the online-softmax combine."""
    errs = {f: F.run_on_gpu(f, T, False, dtype) for f in ("single", "pair")}
    print(f"attn_long_dma_kernel {dtype} T {T}: max |out - ref64| {errs}")


@pytest.mark.parametrize("T", F.DMA_T)
def test_attn_long_dma_kernel_log2e_single(T):
    """attn_long_dma_kernel<true, true> (CLM_ATTN_Q_LOG2E, bf16) on the single family. The intended
    key's log2-domain score is 64 x bf16(log2 e) = 92.5, a bf16 value, so the kernel's bf16 shift equals
    it, P is exactly 1 and the answer exact."""
    err = F.run_on_gpu("single", T, False, "bfloat16", log2e=True)
    print(f"attn_long_dma_kernel bfloat16-log2e T {T}: max |out - ref64| {{'single': {err}}}")


@pytest.mark.parametrize("T", F.DMA_T)
def test_attn_long_dma_kernel_log2e_pair(T):
    """attn_long_dma_kernel<true, true> on the pair family, at the same half-ulp bar.

    The folded form keeps its running shift m as a bf16 value, so the two intended keys' P = exp2(s - m)
    is 1 only when their log2-domain score s = 185 (64 + k_a.k_b) / 64 is itself a bf16 value (k_a.k_b
    = 0; so is all of the single family). Otherwise P loses bits when it is packed to bf16 for the PV
    MFMA. This test found the row sum adding the unrounded fp32 p instead: O / l was off by bf16(p) / p
    and more than half of all rows came out one bf16 ulp off (max |out - ref64| 0.0625 on answers in
    [8, 16)). The kernel now sums the packed P, and both keys weigh exactly the same in O and in l."""
    err = F.run_on_gpu("pair", T, False, "bfloat16", log2e=True)
    print(f"attn_long_dma_kernel bfloat16-log2e T {T}: max |out - ref64| {{'pair': {err}}}")


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
@pytest.mark.parametrize("T", F.CAUSAL_LONG_T)
def test_attn_kernel_causal_families(dtype, T):
    """attn_kernel<*, true> (causal, T > 128), all three families: the per-block nkt, the mask inside
    the diagonal tile (causal_pairs: off by one either way moves a row by 0.5), the combine across
    tiles (pair: a on the diagonal, b in another tile)."""
    errs = {f: F.run_on_gpu(f, T, True, dtype) for f in F.FAMILIES}
    print(f"attn_kernel<causal> {dtype} T {T}: max |out - ref64| {errs}")


def test_attn_long_variants():
    """The three T > 128 non-causal kernels that only $CLM_ATTN_LONG = 0, 1, 2 selects (attn_kernel<*,
    false>, attn_long_kernel<*, false>, attn_long_kernel<*, true>), each in a fresh child process
    (tests/attn_mode_worker.py; the switch is read once per process), one after the other: single and
    pair at T = 129 ... 577 in both dtypes, the Gaussian key-ramp cases that drive their rescale paths,
    and CLM_ATTN_Q_LOG2E refused. Mode 2 is no mere A/B leftover: it is the dispatcher's fallback for
    sequences that attn_long_dma_kernel's 32-bit offsets cannot cover (T > 65535, or a sequence's
    rows spanning 2^31 bytes), which no test-sized shape reaches any other way."""
    for mode in ("0", "1", "2"):
        p = subprocess.run([sys.executable, os.path.join(REPO, "tests", "attn_mode_worker.py")],
                           env=dict(os.environ, CLM_ATTN_LONG=mode), capture_output=True, text=True, timeout=300)
        print(p.stdout, end="")
        assert p.returncode == 0, (mode, p.stdout[-2000:], p.stderr[-3000:])
        assert f"mode {mode} ok" in p.stdout


@pytest.fixture(scope="module")
def ln_inputs():
    """per d: x [301, d] inside a [301, d + 4] buffer (lds = d + 4), gamma, beta and the fp64 LayerNorm"""
    made = {}

    def get(d):
        if d not in made:
            g = torch.Generator(device="cuda").manual_seed(d + 1)
            buf = torch.randn((301, d + 4), generator=g, device="cuda") * 3 + torch.randn((301, 1), generator=g,
                                                                                         device="cuda") * 5
            gam, bet = torch.randn(d, generator=g, device="cuda"), torch.randn(d, generator=g, device="cuda")
            ref = torch.nn.functional.layer_norm(buf[:, :d].double(), (d,), gam.double(), bet.double(), 1e-5)
            made[d] = (buf, gam, bet, ref)
        return made[d]
    return get


def _ln_into(dtype, buf, d, M, gam, bet, y):
    ct = {"bfloat16": C.CLM_BF16, "float16": C.CLM_F16}[dtype]
    return C.lib().clm_layernorm(0, ct, C.ptr(buf), buf.stride(0), M, d, C.ptr(gam), C.ptr(bet), 1e-5, C.ptr(y),
                                 y.stride(0), C.stream_of(buf.device))


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
@pytest.mark.parametrize("d", [128, 256, 512, 768, 1024])
def test_layernorm_variants_strides_and_bounds(dtype, d, ln_inputs):
    """clm_layernorm against fp64 torch LayerNorm at every compiled width -- ln_kernel<*, 1> (d = 128)
    and ln4_kernel<*, 1> (d = 256) included -- with a strided source (lds = d + 4), row counts that
    leave a wave one row of its pair or none (1, 2, 7, 8, 9, 301) and ldy = d, d + 4 (ldy % 8 != 0: the
    8-B store branch even for complete row pairs), d + 8. Bar: one ulp of the type, relative, + 1e-6.
    Columns past d and rows past M keep their sentinel, and a row's bits do not depend on M or ldy."""
    td = {"bfloat16": torch.bfloat16, "float16": torch.float16}[dtype]
    ulp = 2.0 ** (-8 if dtype == "bfloat16" else -11)
    buf, gam, bet, ref = ln_inputs(d)
    first = None
    for M in (301, 1, 2, 7, 8, 9):
        for ldy in (d, d + 4, d + 8):
            y = torch.full((M + 3, ldy), -99.0, device="cuda").to(td)
            C.check(_ln_into(dtype, buf, d, M, gam, bet, y), "clm_layernorm")
            assert (y[M:].float() == -99.0).all() and (y[:, d:].float() == -99.0).all(), (M, ldy)
            got = y[:M, :d]
            err = (got.double() - ref[:M]).abs()
            assert (err <= ulp * ref[:M].abs() + 1e-6).all(), (M, ldy, float(err.max()))
            if first is None:
                first = got.clone()
            assert torch.equal(got, first[:M]), (M, ldy)


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_layernorm_uncompiled_width_is_an_error(dtype, ln_inputs):
    """d = 384 passes the hook's argument check (a multiple of 128, <= 1024) but no kernel is compiled
    for it: an error code, nothing written, and the next call works."""
    td = {"bfloat16": torch.bfloat16, "float16": torch.float16}[dtype]
    buf, gam, bet, _ = ln_inputs(512)
    y = torch.full((9, 512), -99.0, device="cuda").to(td)
    assert _ln_into(dtype, buf, 384, 9, gam, bet, y) != C.CLM_OK
    torch.cuda.synchronize()
    assert (y.float() == -99.0).all()
    C.check(_ln_into(dtype, buf, 512, 9, gam, bet, y), "clm_layernorm")
    torch.cuda.synchronize()
    assert (y.float() != -99.0).all()
