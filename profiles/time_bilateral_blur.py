"""Times bilateral_blur on the device against three baselines measured in the same run:

    python profiles/time_bilateral_blur.py [--out profiles/r09_bilateral_blur.json] [--batch 64] [--size 512]

Configurations: B x 3 x S x S (default 64 x 3 x 512^2), float32 and bfloat16, windows 5 and 9, l1, reflect border, forward and forward + backward.
Each configuration runs in a process of its own under its own `timeout`; the steps are chained - the first one that fails, is killed or times
out ends the run (nothing more is started on the device) and the file records which.  Per configuration, device-event times (warm-up, then
the median of the repeats) of

  * native          kornia_amd.filters.bilateral_blur (km_bilateral_blur_fwd / _bwd);
  * copy            km_stream_copy of the image's bytes (read once + write once: what the operation has to move);
  * gaussian        kornia_amd.filters.gaussian_blur2d at the same window (the package's separable blur, the same bytes);
  * torch_unfold    the reference's algorithm restated in torch on the same device (pad, unfold, the elementwise passes, two sums), or the
                    reason it did not run (out of memory under the cap of half the device).

The speed of the native op is judged against torch_unfold, copy and gaussian - never against an earlier run of itself."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMA_SPACE = (1.5, 1.5)
SIGMA_COLOR = 0.1
STEP_TIMEOUT = 150  # seconds per configuration


def configs():
    return [(dt, k, mode) for dt in ("float32", "bfloat16") for k in (5, 9) for mode in ("fwd", "fwd+bwd")]


def torch_unfold(x, k, sigma_color, sigma_space, space):
    """kornia/filters/bilateral.py:60-83 restated: self-guided, l1, reflect"""
    import torch.nn.functional as F

    p = k // 2
    unf = F.pad(x, (p, p, p, p), mode="reflect").unfold(2, k, 1).unfold(3, k, 1).flatten(-2)
    diff = unf - x.unsqueeze(-1)
    colour = (-0.5 / sigma_color**2 * diff.abs().sum(1, keepdim=True).square()).exp()
    kernel = space.view(-1, 1, 1, 1, k * k) * colour
    return (unf * kernel).sum(-1) / kernel.sum(-1)


def one(dtype_name: str, k: int, mode: str, B: int, S: int) -> dict:
    import torch

    sys.path.insert(0, ROOT)
    import kornia_amd as K
    from kornia_amd import _native as N

    assert torch.cuda.is_available(), "a timing needs the device (no fallback)"
    torch.cuda.set_per_process_memory_fraction(0.5)
    dt = getattr(torch, dtype_name)
    dev = torch.device("cuda", 0)
    x = torch.rand(B, 3, S, S, generator=torch.Generator().manual_seed(0)).to(dt).to(dev)
    go = torch.rand(B, 3, S, S, generator=torch.Generator().manual_seed(1)).to(dt).to(dev)
    bwd = mode == "fwd+bwd"

    def timed(fn, warm=3, reps=15):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "repeats": reps}

    def step(op):
        if not bwd:
            return lambda: op(x)

        def f():
            xg = x.detach().requires_grad_()
            op(xg).backward(go)
        return f

    res = {"dtype": dtype_name, "kernel": k, "mode": mode, "shape": [B, 3, S, S], "sigma_color": SIGMA_COLOR, "sigma_space": list(SIGMA_SPACE),
           "image_bytes": x.numel() * x.element_size(), "device": torch.cuda.get_device_name(0)}
    res["native"] = timed(step(lambda t: K.filters.bilateral_blur(t, k, SIGMA_COLOR, SIGMA_SPACE, "reflect", "l1")))
    res["gaussian"] = timed(step(lambda t: K.filters.gaussian_blur2d(t, (k, k), SIGMA_SPACE, "reflect")))
    dst = torch.empty_like(x)
    nbytes, stream = x.numel() * x.element_size(), N.stream_ptr(dev)
    res["copy"] = timed(lambda: N.check(N.lib().km_stream_copy(x.data_ptr(), dst.data_ptr(), nbytes, 1, stream), "km_stream_copy"))
    space = K.filters.get_gaussian_kernel2d((k, k), SIGMA_SPACE, dtype=dt).to(dev)
    try:
        res["torch_unfold"] = timed(step(lambda t: torch_unfold(t, k, SIGMA_COLOR, SIGMA_SPACE, space)), warm=1, reps=3)
        # the same inputs, the two results side by side (float32: the project's fp32 bound; 16-bit: the reference rounds every intermediate)
        with torch.no_grad():
            n = min(B, 2)
            d = (K.filters.bilateral_blur(x[:n], k, SIGMA_COLOR, SIGMA_SPACE).float() - torch_unfold(x[:n], k, SIGMA_COLOR, SIGMA_SPACE, space).float()).abs().max().item()
        res["max_abs_diff_vs_torch_unfold"] = d
    except torch.cuda.OutOfMemoryError as e:
        res["torch_unfold"] = {"did_not_run": "out of memory under a cap of half the device's memory", "detail": str(e).splitlines()[0][:200]}
    for name in ("copy", "gaussian", "torch_unfold"):
        if "median_ms" in res[name]:
            res[f"native_over_{name}"] = res["native"]["median_ms"] / res[name]["median_ms"]
    return res


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_bilateral_blur.json"))
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--one", nargs=3, metavar=("DTYPE", "K", "MODE"))
    a = ap.parse_args()
    if a.one:
        print("RESULT " + json.dumps(one(a.one[0], int(a.one[1]), a.one[2], a.batch, a.size)), flush=True)
        return 0
    out = {"what": "bilateral_blur on the device against km_stream_copy, gaussian_blur2d and the reference's algorithm in torch (profiles/time_bilateral_blur.py)",
           "results": [], "ended": "complete"}
    rc = 0
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def write(ended):
        with open(a.out, "w") as f:
            json.dump({**out, "ended": ended}, f, indent=1)

    for dt, k, mode in configs():
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT), sys.executable, os.path.abspath(__file__), "--one", dt, str(k), mode, "--batch", str(a.batch), "--size", str(a.size)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        line = next((ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")), None)
        if p.returncode != 0 or line is None:  # a failure, a fault or a time limit: nothing more is started
            out["ended"] = f"stopped at {dt} {k} {mode}: exit status {p.returncode}"
            out["stderr_tail"] = p.stderr[-2000:]
            rc = 1
            break
        out["results"].append(json.loads(line[len("RESULT "):]))
        print(line, flush=True)
        write(f"in progress: {len(out['results'])} of {len(configs())} configurations")  # (what was measured survives a limit on the whole run)
    write(out["ended"])
    print(a.out, out["ended"])
    return rc


if __name__ == "__main__":
    sys.exit(main())
