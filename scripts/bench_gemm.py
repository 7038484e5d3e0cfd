"""GEMM microbenchmark: the MFMA GEMM of csrc/gemm.hip vs torch.matmul (hipBLASLt)
on the three Linear-layer layouts, bf16 and f32.  Prints one JSON line per case."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_training_pytorch_amd.ops.gemm import gemm  # noqa: E402

DEV = torch.device("cuda", 0)


def timeit(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def case(M, N, K, ta, tb, dtype, iters):
    a = (torch.rand(*((K, M) if ta else (M, K)), device=DEV) * 2 - 1).to(dtype)  # uniform [-1, 1): DVFS-honest
    b = (torch.rand(*((K, N) if tb else (N, K)), device=DEV) * 2 - 1).to(dtype)
    out = torch.empty(M, N, device=DEV, dtype=torch.float32 if ta else dtype)
    A = a.t() if ta else a
    Bt = b if tb else b.t()  # [K, N]
    ours = timeit(lambda: gemm(a, b, trans_a=ta, trans_b=tb, out=out), iters)
    classic = timeit(lambda: gemm(a, b, trans_a=ta, trans_b=tb, out=out, fast=False), iters)
    theirs = timeit(lambda: torch.matmul(A, Bt), iters)
    gemm(a, b, trans_a=ta, trans_b=tb, out=out)
    err = (out.float() - torch.matmul(A.float(), Bt.float())).abs().max().item()
    fl = 2.0 * M * N * K
    return {"M": M, "N": N, "K": K, "layout": f"{'T' if ta else 'N'}{'T' if tb else 'N'}", "dtype": str(dtype),
            "ours_ms": round(ours, 4), "ours_tflops": round(fl / ours / 1e9, 1),
            "classic_tflops": round(fl / classic / 1e9, 1),
            "torch_ms": round(theirs, 4), "torch_tflops": round(fl / theirs / 1e9, 1), "max_abs_err": err}


def fp8_layers(widths, batch, rounds, iters):
    """--fp8: the three layer GEMMs of a W-wide Linear at bench_wide.py's batch (forward, dx, dW)
    on the FP8 kernel, both matrix instructions (f8f6f4 16x16x128 / fp8 16x16x32), interleaved
    with the bf16 kernels of the same build in one process: `rounds` rounds, medians.  Then the
    quantiser alone: GB/s against the bytes it moves (x read, q and qT written)."""
    from distributed_training_pytorch_amd.ops.fp8 import Fp8DelayedState, gemm_fp8, quantize_fp8

    def rnd(*shape):
        return torch.rand(*shape, device=DEV) * 2 - 1

    for W in widths:
        h, w, dz = rnd(batch, W).bfloat16(), rnd(W, W), rnd(batch, W).bfloat16()
        wb = w.bfloat16()
        hq, wq, dq = (quantize_fp8(h, "e4m3", True), quantize_fp8(w, "e4m3", True), quantize_fp8(dz, "e5m2", True))
        bias, dwf = rnd(W), torch.zeros(W, W, device=DEV)
        fns = {"fwd": {"bf16": lambda: gemm(h, wb, bias=bias, act=True)},
               "dx": {"bf16": lambda: gemm(dz, wb, trans_b=True, aux=h)},
               "dW": {"bf16": lambda: gemm(dz, h, trans_a=True, trans_b=True, out=dwf, accumulate=True)}}
        for m, tag in ((0, "fp8_x128"), (1, "fp8_x32")):
            fns["fwd"][tag] = lambda m=m: gemm_fp8(hq, wq, bias=bias, act=True, mfma=m)
            fns["dx"][tag] = lambda m=m: gemm_fp8(dq, wq, trans_b=True, aux=h, mfma=m)
            fns["dW"][tag] = lambda m=m: gemm_fp8(dq, hq, trans_a=True, trans_b=True, out=dwf, accumulate=True, mfma=m)
        # delayed scaling: the same GEMMs emitting their output quantised (both copies, amax) from the epilogue,
        # and the given-scale quantiser launch that an unfused output would need instead
        st = Fp8DelayedState(2, device=DEV)
        st.set_scale(0, 448.0 / W, "e4m3")
        st.set_scale(1, 57344.0 / W, "e5m2")
        fns["fwd"]["fp8_x128_qout"] = lambda: gemm_fp8(hq, wq, bias=bias, act=True, quant_out=("e4m3", st.slot(0)))
        fns["dx"]["fp8_x128_qout"] = lambda: gemm_fp8(dq, wq, trans_b=True, aux=h, quant_out=("e5m2", st.slot(1)))
        fns["fwd"]["quantize_scaled"] = lambda: quantize_fp8(h, "e4m3", True, scale=st.slot(0))
        fns["dx"]["quantize_scaled"] = lambda: quantize_fp8(dz, "e5m2", True, scale=st.slot(1))
        fns["fwd"]["quantize_current"] = lambda: quantize_fp8(h, "e4m3", True)
        fns["dx"]["quantize_current"] = lambda: quantize_fp8(dz, "e5m2", True)
        # the planned split-K dW (fp8_x128, where a plan exists) next to the same GEMM unsplit
        fns["dW"]["fp8_x128_unsplit"] = lambda: gemm_fp8(dq, hq, trans_a=True, trans_b=True, out=dwf, accumulate=True,
                                                         split_k=1)
        for name, impls in fns.items():
            ms = {k: [] for k in impls}
            for _ in range(rounds):
                for k, fn in impls.items():
                    ms[k].append(timeit(fn, iters))
            med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
            fl = 2.0 * batch * W * W
            print(json.dumps({"gemm": name, "W": W, "batch": batch, "rounds": rounds,
                              **{f"{k}_ms": round(v, 4) for k, v in med.items()},
                              **{f"{k}_tflops": round(fl / v / 1e9, 1) for k, v in med.items()
                                 if not k.startswith("quantize")}}), flush=True)
        for x, fmt in ((h, "e4m3"), (w, "e4m3"), (dz, "e5m2")):
            t = sorted(timeit(lambda: quantize_fp8(x, fmt, True), iters) for _ in range(rounds))[rounds // 2]
            nbytes = x.numel() * (x.element_size() + 2)
            print(json.dumps({"quantize": fmt, "shape": list(x.shape), "in": str(x.dtype), "ms": round(t, 4),
                              "GB_per_s": round(nbytes / t / 1e6, 1)}), flush=True)


def mxfp8_layers(widths, batch, rounds, iters):
    """--mxfp8: forward / dx / dW of a W-wide Linear at bench_wide.py's batch on the bf16, the
    per-tensor FP8 and the MXFP8 kernels, interleaved in one process (`rounds` rounds, medians),
    then both quantisers (both copies): ms and GB/s against x read plus q and qT written."""
    from distributed_training_pytorch_amd.ops.fp8 import gemm_fp8, quantize_fp8
    from distributed_training_pytorch_amd.ops.mxfp8 import gemm_mxfp8, quantize_mxfp8

    def rnd(*shape):
        return torch.rand(*shape, device=DEV) * 2 - 1

    def median(fns):
        ms = {k: [] for k in fns}
        for _ in range(rounds):
            for k, fn in fns.items():
                ms[k].append(timeit(fn, iters))
        return {k: sorted(v)[len(v) // 2] for k, v in ms.items()}

    for W in widths:
        h, w, dz = rnd(batch, W).bfloat16(), rnd(W, W), rnd(batch, W).bfloat16()
        wb = w.bfloat16()
        hq, wq, dq = (quantize_fp8(h, "e4m3", True), quantize_fp8(w, "e4m3", True), quantize_fp8(dz, "e5m2", True))
        hm, wm, dm = (quantize_mxfp8(t, "e4m3", True) for t in (h, w, dz))
        bias, dwf = rnd(W), torch.zeros(W, W, device=DEV)
        fns = {"fwd": {"bf16": lambda: gemm(h, wb, bias=bias, act=True),
                       "fp8": lambda: gemm_fp8(hq, wq, bias=bias, act=True),
                       "mxfp8": lambda: gemm_mxfp8(hm, wm, bias=bias, act=True)},
               "dx": {"bf16": lambda: gemm(dz, wb, trans_b=True, aux=h),
                      "fp8": lambda: gemm_fp8(dq, wq, trans_b=True, aux=h),
                      "mxfp8": lambda: gemm_mxfp8(dm, wm, trans_b=True, aux=h)},
               "dW": {"bf16": lambda: gemm(dz, h, trans_a=True, trans_b=True, out=dwf, accumulate=True),
                      "fp8": lambda: gemm_fp8(dq, hq, trans_a=True, trans_b=True, out=dwf, accumulate=True),
                      "mxfp8": lambda: gemm_mxfp8(dm, hm, trans_a=True, trans_b=True, out=dwf, accumulate=True),
                      # the planned split-K dW (above, where a plan exists) next to the same GEMMs unsplit
                      "fp8_unsplit": lambda: gemm_fp8(dq, hq, trans_a=True, trans_b=True, out=dwf, accumulate=True,
                                                      split_k=1),
                      "mxfp8_unsplit": lambda: gemm_mxfp8(dm, hm, trans_a=True, trans_b=True, out=dwf, accumulate=True,
                                                          split_k=1)}}
        for name, impls in fns.items():
            med = median(impls)
            fl = 2.0 * batch * W * W
            print(json.dumps({"gemm": name, "W": W, "batch": batch, "rounds": rounds,
                              **{f"{k}_ms": round(v, 4) for k, v in med.items()},
                              **{f"{k}_tflops": round(fl / v / 1e9, 1) for k, v in med.items()}}), flush=True)
    for x in (rnd(8192, 4096).bfloat16(), rnd(4096, 4096)):
        med = median({"fp8": lambda: quantize_fp8(x, "e4m3", True), "mxfp8": lambda: quantize_mxfp8(x, "e4m3", True)})
        nbytes = x.numel() * (x.element_size() + 2)
        print(json.dumps({"quantize": list(x.shape), "in": str(x.dtype), "rounds": rounds,
                          **{f"{k}_ms": round(v, 4) for k, v in med.items()},
                          **{f"{k}_GB_per_s": round(nbytes / v / 1e6, 1) for k, v in med.items()}}), flush=True)


def main():
    if "--mxfp8" in sys.argv:
        return mxfp8_layers((1024, 2048, 4096), 8192, 5, 10)
    if "--fp8" in sys.argv:
        return fp8_layers((1024, 2048, 4096), 8192, 5, 10)
    cases = [(4096, 4096, 4096), (8192, 8192, 8192), (8192, 4096, 4096), (16384, 1024, 1024)]
    dtypes = ((torch.bfloat16, 20),) if "--bf16" in sys.argv else ((torch.bfloat16, 20), (torch.float32, 5))
    for dtype, its in dtypes:
        for (M, N, K) in cases:
            if dtype == torch.float32 and M * N * K > 4096 ** 3:
                continue
            for ta, tb in ((False, False), (False, True), (True, True)):
                print(json.dumps(case(M, N, K, ta, tb, dtype, its)), flush=True)


if __name__ == "__main__":
    main()
