"""Worker of tests/test_gpu_attention.py::test_attn_long_variants: one process per value of
CLM_ATTN_LONG (the library reads it once), given in the environment by the parent. It runs the T > 128
non-causal kernel that value selects -- 0: attn_kernel<*, false>, 1: attn_long_kernel<*, false>,
2: attn_long_kernel<*, true> -- on the exact-answer families and on the Gaussian key-ramp cases of
test_attention_vs_torch, confirms that the log2(e) form of q is refused there, prints one line per
group and exits non-zero with a message at the first failure."""
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import attn_families as F  # noqa: E402
from clip_lora_match_amd import _capi as C  # noqa: E402

DT = {"bfloat16": (torch.bfloat16, C.CLM_BF16, 3e-2), "float16": (torch.float16, C.CLM_F16, 4e-3)}


def gaussian_ramp(dtype, B, T, H, ramp):
    """inputs, fp32 torch reference and bar of test_gpu_kernels.py::test_attention_vs_torch"""
    td, ct, bar = DT[dtype]
    g = torch.Generator(device="cuda").manual_seed(T * H)
    qkv = torch.randn((B * T, 3 * H * 64), generator=g, device="cuda")
    qkv[:, : H * 64] *= 0.125 * 3
    t = torch.linspace(0.0, 1.0, T, device="cuda").repeat(B)
    f = 0.5 + (2.0 if abs(ramp) == 1 else 12.0) * (t if ramp > 0 else 1.0 - t)
    qkv[:, H * 64: 2 * H * 64] *= f[:, None]
    qkv = qkv.to(td)
    out = torch.full((B * T + 8, H * 64 + 64), 7.0, device="cuda").to(td)
    C.check(C.lib().clm_attention(0, ct, 0, C.ptr(qkv), C.ptr(out), out.stride(0), B, T, H, C.stream_of(qkv.device)),
            "clm_attention")
    x = qkv.float().view(B, T, 3, H, 64)
    q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))
    ref = (torch.softmax(q @ k.transpose(-1, -2), -1) @ v).transpose(1, 2).reshape(B * T, H * 64)
    err = (out[: B * T, : H * 64].float() - ref).abs().max().item()
    assert err < bar, (dtype, B, T, H, ramp, err)
    assert (out[:, H * 64:].float() == 7.0).all() and (out[B * T:].float() == 7.0).all(), (dtype, B, T, H, ramp)
    return err


def main():
    mode = int(os.environ["CLM_ATTN_LONG"])
    assert mode in (0, 1, 2), mode
    for dtype in DT:
        for family in ("single", "pair"):
            worst = max(F.run_on_gpu(family, T, False, dtype) for T in F.MODE_T)
            print(f"mode {mode} {dtype} {family} T {list(F.MODE_T)}: max |out - ref64| {worst:.3e}", flush=True)
        worst = max(gaussian_ramp(dtype, B, T, H, ramp)
                    for B, T, H in ((1, 577, 2), (2, 300, 2)) for ramp in (1, -1, 2))
        print(f"mode {mode} {dtype} gaussian key ramps: max |out - ref32| {worst:.3e}", flush=True)
    # only the default kernel (mode 3) takes q in the log2 domain
    qkv = torch.zeros((577, 3 * 64), dtype=torch.bfloat16, device="cuda")
    out = torch.zeros((577, 64), dtype=torch.bfloat16, device="cuda")
    rc = C.lib().clm_attention_ex(0, C.CLM_BF16, C.CLM_ATTN_Q_LOG2E, C.ptr(qkv), C.ptr(out), 64, 1, 577, 1,
                                  C.stream_of(qkv.device))
    assert rc == C.CLM_E_ARG, f"CLM_ATTN_Q_LOG2E accepted in mode {mode}: rc {rc}"
    torch.cuda.synchronize()
    print(f"mode {mode} ok", flush=True)


if __name__ == "__main__":
    try:
        main()
    except Exception as e:  # noqa: BLE001
        print(f"FAILED (CLM_ATTN_LONG={os.environ.get('CLM_ATTN_LONG')}): {type(e).__name__}: {e}", flush=True)
        sys.exit(1)
