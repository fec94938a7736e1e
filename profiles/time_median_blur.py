"""median_blur on the device against its yardsticks: writes profiles/r08_median_blur.json (or --out) and prints it as one JSON line.

64x3x512^2 in float32 and bfloat16, HIP events, a warm-up, the median of 7 groups of 50 calls (fewer calls per group for anything slower
than 5 ms a call):
  * median_blur 3x3 / 5x5 (the register-tiled kernels) and 7x7 (the generic LDS kernel), forward; forward + backward for 3x3 and 5x5;
  * in the same process: km_stream_copy of the same bytes (plain and non-temporal) - x read once + y written once is what the op needs -,
    the package's box_blur 3x3 / 5x5 on the same tensor (the same 2e bytes and the same tiling), and the reference's algorithm restated
    in torch on the device (one-hot conv2d into a (B C, ky kx, H, W) tensor + median(dim=2)).
GB/s figures are the algorithmic bytes (2 * numel * element size) over the call time.
Usage: python profiles/time_median_blur.py [--groups 7] [--calls 50] [--shape 64 3 512 512] [--out PATH]"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import kornia_amd.filters as KF  # noqa: E402
from kornia_amd import _native as N  # noqa: E402


def timed(fn, groups, calls):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    if s.elapsed_time(e) > 5.0:
        calls = max(3, calls // 10)
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(groups):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(calls):
            fn()
        e.record()
        torch.cuda.synchronize()
        out.append(s.elapsed_time(e) / calls)
    return round(statistics.median(out), 4)


def reference_algorithm(x, k):
    """kornia/filters/median.py:60-72 restated: the one-hot kernel, conv2d, median over the window axis"""
    b, c, h, w = x.shape
    n = k * k
    kernel = torch.eye(n, device=x.device, dtype=x.dtype).view(n, 1, k, k)
    feats = F.conv2d(x.reshape(b * c, 1, h, w), kernel, padding=(k // 2, k // 2), stride=1)
    return feats.view(b, c, n, h, w).median(dim=2)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--shape", type=int, nargs=4, default=[64, 3, 512, 512])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_median_blur.json"))
    ap.add_argument("--no-reference", action="store_true", help="skip the restated reference algorithm (a profiler run does not need it)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this script measures on a HIP device"
    B, C, H, W = a.shape
    lib = N.lib()
    res = {"shape": [B, C, H, W], "unit": "ms", "groups": a.groups, "calls": a.calls, "device": torch.cuda.get_device_name(0)}
    x32 = torch.rand(B, C, H, W, generator=torch.Generator().manual_seed(0))
    for name, dt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
        x = x32.to(dt).cuda()
        y = torch.empty_like(x)
        nbytes = 2 * x.numel() * x.element_size()
        r = {"algorithmic_bytes": nbytes}
        stream = N.stream_ptr(x.device)
        for label, nt in (("stream_copy_plain", 0), ("stream_copy_nontemporal", 1)):
            r[label] = timed(lambda: N.check(lib.km_stream_copy(x.data_ptr(), y.data_ptr(), nbytes // 2, nt, stream), "km_stream_copy"), a.groups, a.calls)
        for k in (3, 5):
            r[f"box_blur_{k}x{k}"] = timed(lambda: KF.box_blur(x, (k, k)), a.groups, a.calls)
        for k in (3, 5, 7):
            r[f"median_blur_{k}x{k}_fwd"] = timed(lambda: KF.median_blur(x, (k, k)), a.groups, a.calls)
        xg = x.clone().requires_grad_()
        gout = torch.rand_like(x)
        for k in (3, 5):
            def fwd_bwd():
                xg.grad = None
                KF.median_blur(xg, (k, k)).backward(gout)

            r[f"median_blur_{k}x{k}_fwd_bwd"] = timed(fwd_bwd, a.groups, a.calls)
        if not a.no_reference:
            with torch.no_grad():
                for k in (3, 5):
                    assert torch.equal(reference_algorithm(x[:2], k), KF.median_blur(x[:2].contiguous(), (k, k)))
                    r[f"reference_algorithm_{k}x{k}"] = timed(lambda: reference_algorithm(x, k), 3, 5)
                    r[f"speedup_over_reference_algorithm_{k}x{k}"] = round(r[f"reference_algorithm_{k}x{k}"] / r[f"median_blur_{k}x{k}_fwd"], 1)
        for k in (3, 5, 7):
            r[f"median_blur_{k}x{k}_fwd_GBps"] = round(nbytes / (r[f"median_blur_{k}x{k}_fwd"] * 1e-3) / 1e9, 1)
        r["stream_copy_nontemporal_GBps"] = round(nbytes / (r["stream_copy_nontemporal"] * 1e-3) / 1e9, 1)
        for k in (3, 5):
            r[f"median_over_box_blur_{k}x{k}"] = round(r[f"median_blur_{k}x{k}_fwd"] / r[f"box_blur_{k}x{k}"], 3)
        res[name] = r
    text = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(text)


if __name__ == "__main__":
    main()
