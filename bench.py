#!/usr/bin/env python
"""Headline benchmark: Mpix/s of one fwd+bwd step of

    y = gaussian_blur2d(warp_perspective(x, M, (512, 512)), (5, 5), (1.5, 1.5));  y.backward(grad_out)

with x (B,3,512,512) fp32 requiring grad and M (B,3,3) requiring grad - BASELINE.json configs[1]
(inputs follow benchmarks/geometry/flagship.py:89-107 of the reference: uniform-noise images, image quad
perturbed by 8*randn).  Batches shard across GPUs with no data-path collective.

    python bench.py                      # 1 GPU, B = 256, prints ONE JSON line
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W [--scaling strong] [--gather p2p]

  --scaling weak    every rank owns --batch images (default; total work grows with N)
  --scaling strong  --batch images in total, rank r owns its contiguous slice (B = 256 over N GPUs)
  --gather MODE     additionally time the reassembly of the outputs on every rank (never part of `value`):
                    all_gather | p2p (direct peer exchange) | chunked (compute and exchange overlapped, 4 sub-batches)
  --dump-outputs D  write the last timed step's y, grad wrt x and grad wrt M (rank 0) to D/<name>.npy, float32; the inputs are
                    seeded, so two builds run with the same arguments can be compared output for output
  --full            also measure what the keys below hold; a plain run only sets up, settles (untimed, 3-15 s: first touch of the
                    allocations), runs --warmup steps, times EXACTLY --steps steps (ms_per_step = their wall time / --steps), dumps
                    and prints the headline keys

With --full the JSON line also carries
  ms_per_step_*  after the headline: --groups groups of --steps steps (median, IQR, every group), rotated-input groups
                 interleaved with one-input-set groups; the settle's trace; device clocks before and after
  roofline       the dominant public op of the step (HIP-event timed through the C ABI on the launch stream) against its
                 ALGORITHMIC bytes per SURVEY.md 8(d): warp fwd 2e, blur fwd 2e, blur bwd 2e, warp bwd 3e per element;
                 `kernels` holds every launch with the bytes that launch itself must move
  cpu_baseline   the reference's op sequence on the host cores (thread sweep, median + IQR, benchmarks/common.py:45-60 style)
  generic_gpu    the same op sequence through PyTorch-ROCm's generic kernels (grid chain + F.grid_sample + pad + conv2d) on
                 this GPU: what the north star says not to be
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

# multi-process GPU work on these hosts needs dmabuf IPC (RCCL's peer buffers fail with `hipIpcGetMemHandle: invalid argument` otherwise); the
# driver's environment exports it already - kept here for a launch from a bare shell, before the HIP runtime initialises
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import torch  # noqa: E402

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec, /opt/skills/guides/MI355X_MICROARCH.md (measured streaming copy on these boxes: 6.2 TB/s)
PMC_FILE = next((p for p in (os.path.join(ROOT, "profiles", f"r0{r}_pmc_traffic.json") for r in (6, 5, 4, 3, 2)) if os.path.exists(p)), "")


def csrc_sha256():
    """sha256 over the kernel sources (kornia_amd/csrc/*.hip, *.h, sorted by name): what a PMC measurement is valid for"""
    import hashlib

    h = hashlib.sha256()
    d = os.path.join(ROOT, "kornia_amd", "csrc")
    for f in sorted(os.listdir(d)):
        if f.endswith((".hip", ".h")):
            h.update(f.encode())
            h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()



def measured_streaming_copy(dev, nbytes=1610612736, calls=20):
    """The copy bandwidth of THE BOX THIS LINE RAN ON: km_stream_copy (16 bytes per lane, grid-stride) over `nbytes` = 1.6 GB - the bytes one
    streaming kernel of the step moves - timed with HIP events on the launch stream, min and median of `calls` after 3 warm-up calls, plain and
    non-temporal.  Leases differ by several per cent; this is the datum that says which kind of lease a line came from."""
    from kornia_amd import _native as N

    lib = N.lib()
    src = torch.empty(nbytes // 8, device=dev, dtype=torch.float32).normal_()
    dst = torch.empty_like(src)
    half = src.numel() * 4
    st = torch.cuda.current_stream(dev)
    out = {"bytes_moved_per_call": 2 * half, "calls": calls}
    for name, nt in (("plain", 0), ("nontemporal", 1)):
        ts = []
        for i in range(calls + 3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            N.check(lib.km_stream_copy(src.data_ptr(), dst.data_ptr(), half, nt, N.stream_ptr(dev)), "km_stream_copy")
            e1.record(st)
            e1.synchronize()
            if i >= 3:
                ts.append(e0.elapsed_time(e1))
        ts.sort()
        out[name] = {"ms_min": round(ts[0], 4), "ms_median": round(ts[len(ts) // 2], 4), "GBps_best": round(2 * half / (ts[0] * 1e-3) / 1e9, 1),
                     "GBps_median": round(2 * half / (ts[len(ts) // 2] * 1e-3) / 1e9, 1)}
    del src, dst
    return out


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--batch", type=int, default=256, help="images per GPU (weak scaling) or in total (strong scaling)")
    p.add_argument("--size", type=int, default=512)
    p.add_argument("--channels", type=int, default=3)
    p.add_argument("--scaling", choices=("weak", "strong"), default="weak")
    p.add_argument("--gather", choices=("none", "all_gather", "p2p", "chunked"), default="none",
                   help="also time the reassembly of the outputs on every rank (reported separately)")
    p.add_argument("--full", action="store_true",
                   help="after the headline, also measure everything else the JSON line can carry: settle + --groups timed groups, "
                        "one-input-set groups, clocks, per-launch roofline, streaming copy, generic_gpu, other_configs, cpu_baseline")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="write what the last timed step returned (y, grad wrt x, grad wrt M) as DIR/<name>.npy in float32; an array "
                        "above 16 MB is stored as a fixed, seeded sample of its flattened elements")
    p.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip cpu_baseline")
    p.add_argument("--no-extras", action="store_true", help="with --full: skip other_configs / generic_gpu (profiling runs)")
    p.add_argument("--cpu-batch", type=int, default=8, help="images in the CPU baseline sample")
    p.add_argument("--groups", type=int, default=9,
                   help="with --full: timed groups of --steps steps each (every group bracketed by barrier + synchronize), reported as "
                        "their median, IQR and every group (benchmarks/common.py:45-60 of the reference: median + IQR over blocks)")
    p.add_argument("--input-sets", type=int, default=3,
                   help="distinct (x, M, grad_out) sets rotated through the timed loop: a training loop feeds a new batch every step, so "
                        "nothing of step k's inputs may be found in the 256 MB Infinity Cache by step k+1 (1 = one set, reported beside it)")
    return p.parse_args()


def flagship_homographies(B, H, W, gen):
    """benchmarks/geometry/flagship.py:89-107: M = get_perspective_transform(quad, quad + 8*randn)."""
    src = torch.tensor([[0.0, 0.0], [W - 1.0, 0.0], [W - 1.0, H - 1.0], [0.0, H - 1.0]]).expand(B, 4, 2).double()
    dst = src + 8.0 * torch.randn(B, 4, 2, generator=gen).double()
    A = torch.zeros(B, 8, 8, dtype=torch.float64)
    b = torch.zeros(B, 8, dtype=torch.float64)
    for k in range(4):
        x, y, u, v = src[:, k, 0], src[:, k, 1], dst[:, k, 0], dst[:, k, 1]
        A[:, 2 * k, 0], A[:, 2 * k, 1], A[:, 2 * k, 2] = x, y, 1.0
        A[:, 2 * k, 6], A[:, 2 * k, 7] = -u * x, -u * y
        A[:, 2 * k + 1, 3], A[:, 2 * k + 1, 4], A[:, 2 * k + 1, 5] = x, y, 1.0
        A[:, 2 * k + 1, 6], A[:, 2 * k + 1, 7] = -v * x, -v * y
        b[:, 2 * k], b[:, 2 * k + 1] = u, v
    h = torch.linalg.solve(A, b)
    return torch.cat([h, torch.ones(B, 1, dtype=torch.float64)], dim=1).view(B, 3, 3).float()


def device_clocks(index):
    """Shader clock / power / temperature of torch device `index` from sysfs, read OUTSIDE the timed groups.  The device is found by its PCI
    address (a box may expose the sysfs nodes of GPUs this process cannot use: card0 is not necessarily cuda:0); None where the box does
    not expose it."""
    import glob

    out = {}
    try:
        pr = torch.cuda.get_device_properties(index)
        addr = f"{getattr(pr, 'pci_domain_id', 0):04x}:{pr.pci_bus_id:02x}:{pr.pci_device_id:02x}.0"
        c = os.path.join("/sys/bus/pci/devices", addr)
        if not os.path.exists(os.path.join(c, "pp_dpm_sclk")):
            return {"pci": addr, "note": "no pp_dpm_sclk under this PCI address"}
        out["pci"] = addr
        for line in open(os.path.join(c, "pp_dpm_sclk")):
            if "*" in line:
                out["sclk"] = line.split(":", 1)[1].replace("*", "").strip()
        for line in open(os.path.join(c, "pp_dpm_mclk")):
            if "*" in line:
                out["mclk"] = line.split(":", 1)[1].replace("*", "").strip()
        for hw in glob.glob(os.path.join(c, "hwmon", "hwmon*")):
            for name, key, scale in (("power1_average", "power_W", 1e-6), ("power1_input", "power_W", 1e-6), ("temp1_input", "temp_C", 1e-3),
                                     ("freq1_input", "sclk_MHz_hwmon", 1e-6), ("power1_cap", "power_cap_W", 1e-6)):
                f = os.path.join(hw, name)
                if os.path.exists(f) and key not in out:
                    try:
                        out[key] = round(float(open(f).read().strip()) * scale, 1)
                    except (OSError, ValueError):
                        pass
        try:
            out["busy_percent"] = int(open(os.path.join(c, "gpu_busy_percent")).read().strip())
        except (OSError, ValueError):
            pass
    except (OSError, AttributeError, RuntimeError):
        return out or None
    return out or None


def event_time_ms(fn, iters, repeats=1):
    """Average duration of `fn` (launches on torch's current stream) measured with HIP events on that stream; with repeats > 1 the
    MEDIAN of that many back-to-back samples of `iters` calls."""
    fn()
    torch.cuda.synchronize()
    samples = []
    for _ in range(max(1, repeats)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        samples.append(e0.elapsed_time(e1) / iters)
    samples.sort()
    n = len(samples)
    return samples[n // 2] if n % 2 else 0.5 * (samples[n // 2 - 1] + samples[n // 2])


def kernel_roofline(sets, size, iters):
    """Times every launch of the step and the four public ops by calling the C ABI directly (pre-allocated buffers, no allocator /
    autograd in the timed loop).  Like the step, every timed call works on the NEXT of the input sets (each with its own intermediate
    tensors), under the product's launch policy: nothing a call finds in the 256 MB Infinity Cache was left there by the previous call
    of the loop.  Returns (per-launch stats, per-op stats)."""
    from kornia_amd import _native as N
    from kornia_amd.filters.gaussian import _cached_taps

    lib = N.lib()
    dev = sets[0][0].device
    B, C, H, W = sets[0][0].shape
    h = w = size
    stream = N.stream_ptr(dev)
    kx, ky = _cached_taps(5, 5, (1.5, 1.5), torch.float32, dev)
    n_el = B * C * h * w
    e = 4
    ws_bytes = int(lib.km_warp2d_bwd_workspace_bytes(B, C, H, W, h, w, 1, 0, 0))
    ws = torch.empty(max(ws_bytes, 16), device=dev, dtype=torch.uint8)
    blurred = torch.empty(B, C, h, w, device=dev)  # outputs nobody reads are shared between the sets
    gsrc = torch.empty(B, C, H, W, device=dev)
    gm = torch.zeros(B, 9, device=dev, dtype=torch.float64)
    bufs = []
    for x, M, go in sets:
        x, M = x.detach(), M.detach()
        m = torch.empty(B, 9, device=dev)
        N.check(lib.km_homography_chain_fwd(M.data_ptr(), 3, None, m.data_ptr(), B, H, W, h, w, 0, stream), "chain")
        warped = torch.empty(B, C, h, w, device=dev)
        gw = torch.empty_like(warped)
        N.check(lib.km_warp2d_fwd(x.data_ptr(), m.data_ptr(), warped.data_ptr(), B, C, H, W, h, w, B, 0, 1, 1, 0, 1, None, 0, stream), "wf")
        N.check(lib.km_filter2d_sep_bwd_input(go.data_ptr(), kx.data_ptr(), ky.data_ptr(), gw.data_ptr(), B, C, h, w, 1, 5, 5, 1, 1, 0, stream), "bb")
        bufs.append((x, m, go, warped, gw))
    k = [0]

    def nxt():
        k[0] += 1
        return bufs[k[0] % len(bufs)]

    def warp_fwd():
        x, m, go, warped, gw = nxt()
        N.check(lib.km_warp2d_fwd(x.data_ptr(), m.data_ptr(), warped.data_ptr(), B, C, H, W, h, w, B, 0, 1, 1, 0, 1, None, 0, stream), "wf")

    def blur_fwd():
        x, m, go, warped, gw = nxt()
        N.check(lib.km_filter2d_sep_fwd(warped.data_ptr(), kx.data_ptr(), ky.data_ptr(), blurred.data_ptr(), B, C, h, w, 1, 5, 5, 1, 1, 0, stream), "bf")

    def blur_bwd():
        x, m, go, warped, gw = nxt()
        N.check(lib.km_filter2d_sep_bwd_input(go.data_ptr(), kx.data_ptr(), ky.data_ptr(), gw.data_ptr(), B, C, h, w, 1, 5, 5, 1, 1, 0, stream), "bb")

    def warp_bwd_gsrc():  # tile-owner scatter: grad wrt the image only
        x, m, go, warped, gw = nxt()
        N.check(lib.km_warp2d_bwd(gw.data_ptr(), x.data_ptr(), m.data_ptr(), gsrc.data_ptr(), None, B, C, H, W, h, w, B, 0, 1, 1, 0, 1, None, 0, stream), "wb")

    def warp_bwd_gmat():  # forward-shaped reduction: grad wrt the homography only
        x, m, go, warped, gw = nxt()
        N.check(lib.km_warp2d_bwd(gw.data_ptr(), x.data_ptr(), m.data_ptr(), None, gm.data_ptr(), B, C, H, W, h, w, B, 0, 1, 1, 0, 1, None, 0, stream), "wm")

    def warp_bwd_two():  # both gradients as two launches (each reads grad_out): the form without a workspace
        x, m, go, warped, gw = nxt()
        N.check(lib.km_warp2d_bwd(gw.data_ptr(), x.data_ptr(), m.data_ptr(), gsrc.data_ptr(), gm.data_ptr(), B, C, H, W, h, w, B, 0, 1, 1, 0, 1, None, 0, stream), "wb")

    def warp_bwd():  # the public op as the Python layer calls it: with a workspace, both gradients from one read of grad_out
        x, m, go, warped, gw = nxt()
        N.check(lib.km_warp2d_bwd_ws(gw.data_ptr(), x.data_ptr(), m.data_ptr(), gsrc.data_ptr(), gm.data_ptr(), B, C, H, W, h, w, B, 0, 1, 1, 0, 1, None, 0,
                                     ws.data_ptr() if ws_bytes else None, ws_bytes, stream), "wb")

    fused = bool(ws_bytes) and lib.km_config_get(b"warp_bwd_fused") == 1
    # per LAUNCH: the bytes that launch itself must move (every tensor it reads once + every tensor it writes once)
    kernels = {}
    launches = [
        ("km_warp_fwd_box_kernel", warp_fwd, 2 * e * n_el, "read src, write out"),
        ("km_blur_reg_kernel<fwd>", blur_fwd, 2 * e * n_el, "read x, write y"),
        ("km_blur_reg_kernel<bwd>", blur_bwd, 2 * e * n_el, "read grad_y, write grad_x"),
        ("km_warp_bwd_tiled_kernel", warp_bwd_gsrc, 2 * e * n_el, "read grad_out, write grad_src (the image gradient alone)"),
        ("km_warp_gm_kernel", warp_bwd_gmat, 2 * e * n_el, "read grad_out, read src (the matrix gradient alone)"),
    ]
    if fused:
        launches.append(("km_warp_bwd_fused_kernel (+ boxes, general)", warp_bwd, 3 * e * n_el, "read grad_out, read src, write grad_src: both gradients"))
    for name, fn, nbytes, what in launches:
        ms = event_time_ms(fn, iters, 5)
        kernels[name] = {"ms": round(ms, 4), "launch_bytes": nbytes, "GBps": round(nbytes / ms / 1e6, 1), "moves": what}
    # per PUBLIC OP: SURVEY 8(d)'s algorithmic bytes (compulsory traffic at the API boundary)
    ops = {}
    for name, fn, mult in (("km_warp2d_fwd", warp_fwd, 2), ("km_filter2d_sep_fwd", blur_fwd, 2), ("km_filter2d_sep_bwd_input", blur_bwd, 2),
                           ("km_warp2d_bwd", warp_bwd, 3)):
        ms = kernels["km_warp_fwd_box_kernel"]["ms"] if name == "km_warp2d_fwd" else (
            kernels["km_blur_reg_kernel<fwd>"]["ms"] if name == "km_filter2d_sep_fwd" else (
                kernels["km_blur_reg_kernel<bwd>"]["ms"] if name == "km_filter2d_sep_bwd_input" else event_time_ms(fn, iters, 5)))
        nbytes = mult * e * n_el
        ops[name] = {"ms": round(ms, 4), "alg_bytes": nbytes, "GBps": round(nbytes / ms / 1e6, 1), "frac_of_hbm_peak": round(nbytes / ms / 1e6 / HBM_PEAK_GBS, 4)}
    ops["km_warp2d_bwd"]["form"] = "one read of grad_out (km_warp2d_bwd_ws with a workspace)" if fused else "two launches"
    ops["km_warp2d_bwd"]["ms_two_launches"] = round(event_time_ms(warp_bwd_two, iters, 3), 4)
    ops["km_warp2d_bwd"]["timing"] = f"{len(bufs)} input sets rotated: no call starts on what the previous call of the loop left in the Infinity Cache"
    return kernels, ops


def generic_torch_step_factory():
    """The reference's op sequence for the headline step written with plain torch ops (what kornia executes on a GPU today:
    normalise / invert the homography, build the (B,h,w,2) grid, F.grid_sample, reflect-pad + depthwise conv2d twice)."""
    import torch.nn.functional as F

    def inv3(m):
        a, b, c = m[..., 0], m[..., 1], m[..., 2]
        bc, ca, ab = torch.linalg.cross(b, c), torch.linalg.cross(c, a), torch.linalg.cross(a, b)
        det = (a * bc).sum(-1, keepdim=True)
        return torch.stack([bc, ca, ab], dim=-2) / det[..., None]

    def npix(hh, ww, dev):
        return torch.tensor([[2.0 / (ww - 1), 0.0, -1.0], [0.0, 2.0 / (hh - 1), -1.0], [0.0, 0.0, 1.0]], device=dev)[None]

    def step(x, M, go, S):
        x = x.detach().requires_grad_()
        M = M.detach().requires_grad_()
        dev = x.device
        A = npix(S, S, dev) @ (M @ inv3(npix(x.shape[-2], x.shape[-1], dev)))
        m = inv3(A)
        ys, xs = torch.meshgrid(torch.linspace(-1, 1, S, device=dev), torch.linspace(-1, 1, S, device=dev), indexing="ij")
        u, v = xs[None], ys[None]
        den = m[:, 2, 0, None, None] * u + m[:, 2, 1, None, None] * v + m[:, 2, 2, None, None]
        gx = (m[:, 0, 0, None, None] * u + m[:, 0, 1, None, None] * v + m[:, 0, 2, None, None]) / den
        gy = (m[:, 1, 0, None, None] * u + m[:, 1, 1, None, None] * v + m[:, 1, 2, None, None]) / den
        w = F.grid_sample(x, torch.stack([gx, gy], -1), mode="bilinear", padding_mode="zeros", align_corners=True)
        k = torch.tensor([0.12007838, 0.23388076, 0.29208172, 0.23388076, 0.12007838], device=dev)
        C = x.shape[1]
        y = F.conv2d(F.pad(w, [2, 2, 0, 0], mode="reflect"), k.view(1, 1, 1, 5).expand(C, 1, 1, 5), groups=C)
        y = F.conv2d(F.pad(y, [0, 0, 2, 2], mode="reflect"), k.view(1, 1, 5, 1).expand(C, 1, 5, 1), groups=C)
        y.backward(go)
        return y

    return step


def generic_gpu_baseline(dev, S, C):
    B = 32
    g = torch.Generator().manual_seed(0)
    x = torch.rand(B, C, S, S, generator=g).to(dev)
    M = flagship_homographies(B, S, S, g).to(dev)
    go = torch.rand(B, C, S, S, generator=g).to(dev)
    step = generic_torch_step_factory()
    for _ in range(2):
        step(x, M, go, S)
    torch.cuda.synchronize()
    n, t0 = 5, time.perf_counter()
    for _ in range(n):
        step(x, M, go, S)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / n
    return {"value": round(B * S * S / dt / 1e6, 1), "unit": "Mpix/s", "ms_per_step": round(dt * 1e3, 3),
            "sample": f"B={B}x{C}x{S}x{S} fp32 fwd+bwd, torch {torch.__version__}: grid chain + F.grid_sample + reflect pad + depthwise conv2d (MIOpen)"}


def other_configs(dev):
    """Informational: the parity configurations of BASELINE.json (configs[2..4]) and the callers of the path, timed through the public
    Python API on one GPU (HIP events; median of 7 groups of 50 calls, see `timing`).  Not part of `value`; failures here never affect the bench line."""
    import kornia_amd as K
    import kornia_amd.augmentation as A

    out = {}
    spread = out["timing"] = {"method": "every *_ms below: MEDIAN of 7 groups of 50 calls (HIP events around a group, 5 untimed calls first) - the headline's "
                                        "timed_group scheme; min / max of the groups per figure under `groups_ms`.  Launch-bound sequences (configs 3 and 5: 4 - 10 "
                                        "launches of 5 - 70 us) are quoted as their HIP-graph replay - the kernels' time - with the eager figure, which adds the "
                                        "host's launch gaps, beside it.", "groups_ms": {}}

    def t(fn, label=None, n=50, groups=7):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        samples = []
        for _ in range(groups):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            e1.synchronize()
            samples.append(e0.elapsed_time(e1) / n)
        samples.sort()
        med = samples[len(samples) // 2]
        if label:
            spread["groups_ms"][label] = {"min": round(samples[0], 4), "median": round(med, 4), "max": round(samples[-1], 4)}
        return round(med, 4)

    def roof(ms, alg_bytes):
        """SURVEY.md 8(d) algorithmic bytes of the public ops in the timed sequence / time, as GB/s and fraction of the 8 TB/s HBM peak"""
        return {"ms": ms, "alg_bytes": int(alg_bytes), "GBps": round(alg_bytes / ms / 1e6, 1), "frac_of_hbm_peak": round(alg_bytes / ms / 1e6 / HBM_PEAK_GBS, 4)}

    try:  # config 3: 256 images per GPU, bf16, RandomAffine + ColorJitter + RandomGaussianBlur with device-resident parameters (p = 1)
        with torch.no_grad():
            B = 256
            g = torch.Generator().manual_seed(0)
            x = torch.rand(B, 3, 224, 224, device=dev).bfloat16()
            Pa = {"translations": (torch.rand(B, 2, generator=g) - 0.5) * 44.8, "center": torch.full((B, 2), 111.5), "scale": (0.8 + 0.4 * torch.rand(B, 1, generator=g)).expand(B, 2).contiguous(),
                  "angle": (torch.rand(B, generator=g) - 0.5) * 30, "shear_x": (torch.rand(B, generator=g) - 0.5) * 10, "shear_y": torch.zeros(B)}
            Pj = {"brightness_factor": 0.8 + 0.4 * torch.rand(B, generator=g), "contrast_factor": 0.8 + 0.4 * torch.rand(B, generator=g),
                  "saturation_factor": 0.8 + 0.4 * torch.rand(B, generator=g), "hue_factor": (torch.rand(B, generator=g) - 0.5) * 0.2}
            Pb = {"sigma": 0.1 + 1.9 * torch.rand(B, generator=g)}
            Pa, Pj, Pb = ({k: v.to(dev) for k, v in d.items()} for d in (Pa, Pj, Pb))
            order = [0, 2, 3, 1]

            def seq(xx, a, j, b):
                return A.random_gaussian_blur(A.color_jitter(A.random_affine(xx, a), j, order), b)

            M = A.affine_matrix(Pa, dev)
            w = K.warp_affine(x, M[:, :2], (224, 224), align_corners=False)
            c = A.color_jitter(w, Pj, order)
            out["cfg3_bf16_256x3x224_eager_ms"] = t(lambda: seq(x, Pa, Pj, Pb), "cfg3_eager")
            out["cfg3_breakdown_ms"] = {
                "affine_matrix": t(lambda: A.affine_matrix(Pa, dev)), "warp_affine": t(lambda: K.warp_affine(x, M[:, :2], (224, 224), align_corners=False)),
                "color_jitter": t(lambda: A.color_jitter(w, Pj, order)), "gaussian_blur(per-sample sigma)": t(lambda: A.random_gaussian_blur(c, Pb))}
        step = K.graph.capture(seq, x, Pa, Pj, Pb, no_grad=True)
        out["cfg3_bf16_256x3x224_hip_graph_replay_ms"] = t(step.replay, "cfg3_graph_replay")
        # 3 public ops x 2e, e = 2 bytes (0.462 GB per GPU); the kernels' time = the graph replay (the eager figure beside it)
        out["cfg3_roofline"] = {**roof(min(out["cfg3_bf16_256x3x224_hip_graph_replay_ms"], out["cfg3_bf16_256x3x224_eager_ms"]), 3 * 2 * 2 * x.numel()),
                                "timed": "the faster of HIP-graph replay and eager", "eager_ms": out["cfg3_bf16_256x3x224_eager_ms"]}
    except Exception as e:  # informational only
        out["error_cfg3"] = f"{type(e).__name__}: {e}"
    try:  # config 3 AS BASELINE WRITES IT: AugmentationSequential(RandomAffine, ColorJitter, RandomGaussianBlur)(x), the parameter sampling INSIDE the call
        with torch.no_grad():
            x = torch.rand(256, 3, 224, 224, device=dev).bfloat16()
            aug = A.AugmentationSequential(A.RandomAffine(degrees=15.0, translate=(0.1, 0.1), scale=(0.8, 1.2), shear=5.0, p=1.0),
                                           A.ColorJitter(0.2, 0.2, 0.2, 0.1, p=1.0), A.RandomGaussianBlur((5, 5), (0.1, 2.0), p=1.0))
            torch.manual_seed(0)
            ms_mod = t(lambda: aug(x), "cfg3_as_written_modules_with_sampling")
            # the host's share alone: the three modules' draws (torch's CPU generator, the reference's order) and their three H2D copies
            t0 = time.perf_counter()
            for _ in range(200):
                aug.forward_parameters(x.shape)
            host_ms = (time.perf_counter() - t0) / 200 * 1e3
            rep = aug._params
            ms_replay = t(lambda: aug(x, params=rep), "cfg3_as_written_modules_replay")
        out["cfg3_as_written"] = {
            "call": "kornia_amd.augmentation.AugmentationSequential(RandomAffine(15, (0.1, 0.1), (0.8, 1.2), 5, p=1), ColorJitter(0.2, 0.2, 0.2, 0.1, p=1), RandomGaussianBlur((5, 5), (0.1, 2.0), p=1))(x)",
            "input": "256x3x224x224 bf16 (the per-GPU share of configs[2])",
            "ms_per_call_with_sampling": ms_mod, "ms_per_call_replayed_parameters": ms_replay, "host_sampling_ms_alone": round(host_ms, 4),
            "roofline": roof(ms_mod, 3 * 2 * 2 * x.numel()),
            "note": "the draws are Kornia's own (torch's global CPU generator, same order: tests/test_gpu_aug_modules.py compares them entry for entry with the "
                    "reference's for the same seed); one host buffer and ONE device copy per module; the host works ahead of the device, so the call is "
                    "host-bound only while the host's share per call exceeds the kernels' time",
        }
    except Exception as e:  # informational only
        out["error_cfg3_as_written"] = f"{type(e).__name__}: {e}"
    try:
        with torch.no_grad():
            x = torch.rand(64, 1, 1080, 1920, device=dev)
            R = K.get_rotation_matrix2d(torch.tensor([[959.5, 539.5]], device=dev).repeat(64, 1), torch.full((64,), 2.0, device=dev), torch.ones(64, 2, device=dev))
            out["cfg4_64x1x1080x1920_spatial_gradient_ms"] = t(lambda: K.spatial_gradient(x), "cfg4_spatial_gradient")
            out["cfg4_64x1x1080x1920_warp_affine_bicubic_ms"] = t(lambda: K.warp_affine(x, R, (1080, 1920), mode="bicubic"), "cfg4_bicubic")
            out["cfg4_roofline"] = {"spatial_gradient (3e)": roof(out["cfg4_64x1x1080x1920_spatial_gradient_ms"], 3 * 4 * x.numel()),
                                    "warp_affine bicubic (2e)": roof(out["cfg4_64x1x1080x1920_warp_affine_bicubic_ms"], 2 * 4 * x.numel())}
            del x
        x = torch.rand(128, 3, 256, 256, device=dev)
        H = (torch.eye(3, device=dev)[None] + 0.01 * torch.randn(128, 3, 3, device=dev)).requires_grad_()
        tgt = torch.rand(128, 3, 256, 256, device=dev)

        def learn_h(a, hm, tg):
            (gh,) = torch.autograd.grad(torch.nn.functional.l1_loss(K.homography_warp(a, hm, (256, 256)), tg), hm)
            return gh

        # configs[4]: homography_warp with a learned H, forward + backward wrt H.  THE PATH is homography_warp and its backward: it is timed with the
        # upstream gradient given (like the headline step); the same with torch's l1_loss on top - two thirds of which is torch's loss - beside it
        with torch.no_grad():
            wv = K.homography_warp(x, H, (256, 256))
            bd = {"homography_warp_fwd": t(lambda: K.homography_warp(x, H, (256, 256))), "torch_l1_loss_fwd": t(lambda: torch.nn.functional.l1_loss(wv, tgt))}
        wg = wv.detach().requires_grad_()
        bd["torch_l1_loss_fwd+bwd"] = t(lambda: torch.autograd.grad(torch.nn.functional.l1_loss(wg, tgt), wg))
        go5 = torch.rand_like(wv)

        def warp_fb():
            (gh,) = torch.autograd.grad(K.homography_warp(x, H, (256, 256)), H, go5)
            return gh

        out["cfg5_128x3x256x256_homography_warp_fwd+gradH_eager_ms"] = bd["homography_warp_fwd+gradH"] = t(warp_fb, "cfg5_fwd+gradH_eager")
        bd["gradH_only (fwd+gradH minus fwd)"] = round(bd["homography_warp_fwd+gradH"] - bd["homography_warp_fwd"], 4)
        out["cfg5_128x3x256x256_l1(homography_warp)+gradH_eager_ms"] = bd["l1_loss(homography_warp)+gradH (whole sequence)"] = t(lambda: learn_h(x, H, tgt))
        out["cfg5_breakdown_ms"] = bd

        def warp_fb_g(a, hm, go):
            (gh,) = torch.autograd.grad(K.homography_warp(a, hm, (256, 256)), hm, go)
            return gh

        # the same sequence as a HIP graph: what its kernels take (chain, forward, matrix gradient, chain backward) without the host's launch gaps
        out["cfg5_128x3x256x256_homography_warp_fwd+gradH_hip_graph_replay_ms"] = t(K.graph.capture(warp_fb_g, x, H, go5).replay, "cfg5_fwd+gradH_graph_replay")
        # homography_warp 2e forward + 2e backward wrt H only (0.403 GB per GPU); a loss on top is outside the path
        out["cfg5_roofline"] = {**roof(min(out["cfg5_128x3x256x256_homography_warp_fwd+gradH_hip_graph_replay_ms"], out["cfg5_128x3x256x256_homography_warp_fwd+gradH_eager_ms"]), 4 * 4 * x.numel()),
                                "timed": "homography_warp forward + backward wrt H, upstream gradient given; the faster of HIP-graph replay and eager",
                                "eager_ms": out["cfg5_128x3x256x256_homography_warp_fwd+gradH_eager_ms"]}
        out["cfg5_roofline_with_torch_l1_loss_in_the_timing"] = roof(out["cfg5_128x3x256x256_l1(homography_warp)+gradH_eager_ms"], 4 * 4 * x.numel())
        gstep = K.graph.capture(learn_h, x, H, tgt)
        out["cfg5_128x3x256x256_l1(homography_warp)+gradH_hip_graph_replay_ms"] = t(gstep.replay)
        T = K.geometry.transform

        def fused(a, hm, tg):
            (gh,) = torch.autograd.grad(T.masked_warp_loss(a, tg, hm, threshold=None), hm)
            return gh

        out["cfg5_128x3x256x256_fused_loss+gradH_one_launch_eager_ms"] = t(lambda: fused(x, H, tgt), "cfg5_fused_loss_eager")
        out["cfg5_128x3x256x256_fused_loss+gradH_one_launch_hip_graph_replay_ms"] = t(K.graph.capture(fused, x, H, tgt).replay, "cfg5_fused_loss_graph_replay")
        # the fused op is another public op (masked_warp_loss, the ImageRegistrator's level loss): reads image and target once = 2e
        out["cfg5_fused_loss_roofline"] = {**roof(min(out["cfg5_128x3x256x256_fused_loss+gradH_one_launch_hip_graph_replay_ms"], out["cfg5_128x3x256x256_fused_loss+gradH_one_launch_eager_ms"]), 2 * 4 * x.numel()),
                                           "timed": "the faster of HIP-graph replay and eager"}
        # transform_points well beyond the 256 MB Infinity Cache: 2048 x 65536 x 2 fp32 = 1.07 GB in, 1.07 GB out (2e bytes per coordinate),
        # a fresh output every call; profiles/r03_transform_points_* hold the rocprofv3 kernel stats and FETCH / WRITE sizes of this loop
        P = torch.rand(2048, 65536, 2, device=dev)
        Tm = torch.eye(3, device=dev)[None].repeat(2048, 1, 1) + 0.01 * torch.randn(2048, 3, 3, device=dev)
        with torch.no_grad():
            ms = t(lambda: K.transform_points(Tm, P), "transform_points", n=20)
        out["transform_points_2048x65536x2"] = {**roof(round(ms, 4), 2 * P.numel() * 4), "mfma": "not used: K = 3 contraction, 15 flop per 16 bytes (profiles/README.md)"}
        del P
    except Exception as e:
        out["error_cfg45"] = f"{type(e).__name__}: {e}"
    try:  # the fused warp + blur op (csrc/km_warp_blur.hip), config 2's shapes: a SEPARATE public op, never part of `value`
        B, S = 256, 512
        g = torch.Generator().manual_seed(5)
        gg = torch.Generator(device=dev).manual_seed(5)
        fsets = [(torch.rand(B, 3, S, S, device=dev, generator=gg), flagship_homographies(B, S, S, g).to(dev), torch.rand(B, 3, S, S, device=dev, generator=gg)) for _ in range(2)]
        T = K.geometry.transform
        kk = [0]

        def fstep(fn):
            def f():
                kk[0] += 1
                xs, Ms, gos = fsets[kk[0] % 2]
                xs, Ms = xs.detach().requires_grad_(), Ms.detach().requires_grad_()
                fn(xs, Ms).backward(gos)
            return f

        def ffwd(fn):
            def f():
                kk[0] += 1
                xs, Ms, gos = fsets[kk[0] % 2]
                with torch.no_grad():
                    fn(xs, Ms)
            return f

        fused = lambda a_, m_: T.warp_perspective_blur(a_, m_, (S, S), (5, 5), (1.5, 1.5))
        two = lambda a_, m_: K.gaussian_blur2d(K.warp_perspective(a_, m_, (S, S)), (5, 5), (1.5, 1.5))
        ms_f, ms_t = t(fstep(fused), "fused_warp_blur_fwd+bwd", n=20), t(fstep(two), "two_ops_fwd+bwd", n=20)
        n_el = B * 3 * S * S
        out["fused_warp_blur_256x3x512x512"] = {
            "op": "kornia_amd.geometry.transform.warp_perspective_blur: one forward launch (the warped image never reaches HBM), backward = blur adjoint + one-read warp backward",
            "fwd+bwd_ms": ms_f, "Mpix_s": round(B * S * S / ms_f / 1e3, 1), "two_ops_same_loop_ms": ms_t,
            "forward_only_ms": t(ffwd(fused), n=20), "forward_only_two_ops_ms": t(ffwd(two), n=20),
            "alg_bytes": 7 * 4 * n_el, "accounting": "fused forward 2e + blur adjoint 2e + warp backward 3e = 7e (a fused adjoint would make it 5e; the two ops: 9e)",
            "GBps": round(7 * 4 * n_el / ms_f / 1e6, 1), "frac_of_hbm_peak": round(7 * 4 * n_el / ms_f / 1e6 / HBM_PEAK_GBS, 4),
            "bit_identical_to_two_ops": bool(torch.equal(fused(fsets[0][0][:4], fsets[0][1][:4]), two(fsets[0][0][:4], fsets[0][1][:4]))),
        }
        del fsets
    except Exception as e:  # informational only
        out["error_fused_warp_blur"] = f"{type(e).__name__}: {e}"
    try:  # the pyramid / registration stack and the remaining callers
        T = K.geometry.transform
        with torch.no_grad():
            x = torch.rand(256, 3, 512, 512, device=dev)
            out["pyrdown_256x3x512x512_ms"] = t(lambda: T.pyrdown(x))
            out["build_pyramid_5_levels_256x3x512x512_ms"] = t(lambda: T.build_pyramid(x, 5))
            del x
            x = torch.rand(64, 3, 256, 256, device=dev)
            out["pyrup_64x3x256x256_to_512_ms"] = t(lambda: T.pyrup(x))
            x = torch.rand(16, 3, 512, 512, device=dev)
            out["canny_16x3x512x512_ms"] = t(lambda: K.filters.canny(x))
    except Exception as e:  # informational only
        out["error_callers"] = f"{type(e).__name__}: {e}"
    return out


def cpu_baseline(size, channels, cpu_batch):
    """The reference's CPU path (its torch op sequence, oracle/torch_ref.py) on the host cores of this box, on a bounded sample of
    the same workload: median + IQR per thread count (torch.utils.benchmark blocked_autorange, like benchmarks/common.py:45-60),
    the best thread count is `value`.  Mpix/s is batch-normalised, so the sample batch is stated, not scaled."""
    import torch.utils.benchmark as tbench

    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import torch_ref  # test infrastructure: baseline leg only

    logical = os.cpu_count() or 1
    g = torch.Generator().manual_seed(0)
    x = torch.rand(cpu_batch, channels, size, size, generator=g)
    M = flagship_homographies(cpu_batch, size, size, g)
    go = torch.rand(cpu_batch, channels, size, size, generator=g)
    sweep = {}
    candidates = sorted({min(logical, n) for n in (8, 32, max(1, logical // 2))})
    old = torch.get_num_threads()
    try:
        for nt in candidates:
            torch.set_num_threads(nt)
            torch_ref.headline_step(x, M, go, (size, size))  # warm-up
            m = tbench.Timer(stmt="f(x, M, go, s)", globals={"f": torch_ref.headline_step, "x": x, "M": M, "go": go, "s": (size, size)},
                             num_threads=nt).blocked_autorange(min_run_time=3.0)
            sweep[str(nt)] = {"median_ms": round(m.median * 1e3, 2), "iqr_ms": round(m.iqr * 1e3, 2), "runs": len(m.times),
                              "Mpix_s": round(cpu_batch * size * size / m.median / 1e6, 3)}
    finally:
        torch.set_num_threads(old)
    best = max(sweep, key=lambda k: sweep[k]["Mpix_s"])
    # second CPU figure: the plain-C oracle (OpenMP over the same host cores), fwd + bwd of the same sample
    import oracle as c_oracle

    t1 = time.perf_counter()
    w = c_oracle.warp_perspective(x, M, (size, size))
    c_oracle.gaussian_blur2d(w, (5, 5), (1.5, 1.5))
    gw = c_oracle.gaussian_blur2d_backward(go, w, (5, 5), (1.5, 1.5))
    c_oracle.warp_perspective_backward(gw, x, M, (size, size))
    c_dt = time.perf_counter() - t1
    model = ""
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                model = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    return {
        "value": sweep[best]["Mpix_s"],
        "unit": "Mpix/s",
        "cores": int(best),
        "kind": "port",
        "sample": f"fwd+bwd steps of B={cpu_batch}x{channels}x{size}x{size} fp32 through the reference's PyTorch-CPU op sequence (oracle/torch_ref.py), "
                  f"blocked_autorange >= 3 s per thread count; median {sweep[best]['median_ms']} ms, IQR {sweep[best]['iqr_ms']} ms at {best} threads",
        "host": f"{model}, {logical} logical CPUs",
        "thread_sweep": sweep,
        "c_oracle_value": round(cpu_batch * size * size / c_dt / 1e6, 3),
        "c_oracle_note": f"plain-C oracle (OpenMP, {logical} threads), one fwd+bwd of the same sample in {c_dt:.2f} s",
    }


DUMP_ARRAY_BYTES = 16 << 20  # per array: y and grad_x of the flagship step are 805 MB each; three arrays stay under 64 MB in all


def dump_outputs(out_dir, arrays):
    """Write every array as out_dir/<name>.npy in float32.  An array above DUMP_ARRAY_BYTES is stored as a sample of its flattened
    elements: sorted indices drawn from a generator seeded with the element count, so every run and every build of the same
    arguments picks the same elements."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    for name, t in arrays.items():
        t = t.detach().float()
        keep = DUMP_ARRAY_BYTES // 4
        if t.numel() > keep:
            idx = torch.randint(0, t.numel(), (keep,), generator=torch.Generator().manual_seed(t.numel())).sort().values
            t = t.reshape(-1)[idx.to(t.device)]
        np.save(os.path.join(out_dir, f"{name}.npy"), t.cpu().numpy())


def main():
    args = parse_args()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} must be launched with torch.distributed.run --nproc-per-node {args.gpus} (WORLD_SIZE={world})")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device (no CPU fallback)")
    # test hooks (1-GPU box): BENCH_FORCE_DEVICE=0 maps every rank to one device, BENCH_DIST_BACKEND=gloo replaces RCCL
    force_dev = os.environ.get("BENCH_FORCE_DEVICE")
    dev_index = int(force_dev) if force_dev is not None else local_rank
    backend = os.environ.get("BENCH_DIST_BACKEND", "nccl")  # "nccl" is RCCL on ROCm
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    dist = None
    if world > 1:
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=dev)
        else:
            dist.init_process_group(backend=backend)

    import kornia_amd as K
    from kornia_amd.distributed import gather_batch, shard_bounds

    C, S = args.channels, args.size
    if args.scaling == "strong":
        lo, hi = shard_bounds(args.batch, world, rank)
        B, global_batch = hi - lo, args.batch
    else:
        B, global_batch = args.batch, world * args.batch
    gen = torch.Generator().manual_seed(1000 * rank)
    ggen = torch.Generator(device=dev).manual_seed(1000 * rank)
    n_sets = max(1, args.input_sets)
    sets = []
    for _ in range(n_sets):
        sets.append((torch.rand(B, C, S, S, device=dev, generator=ggen).requires_grad_(), flagship_homographies(B, S, S, gen).to(dev).requires_grad_(),
                     torch.rand(B, C, S, S, device=dev, generator=ggen)))
    x, M, go = sets[0]
    counter = [0]

    def step(fixed_set=None):
        # every step works on the NEXT input set: step k+1 cannot start on what step k left in the Infinity Cache
        xs, Ms, gos = sets[(counter[0] % n_sets) if fixed_set is None else fixed_set]
        counter[0] += 1
        xs.grad = None
        Ms.grad = None
        y = K.gaussian_blur2d(K.warp_perspective(xs, Ms, (S, S)), (5, 5), (1.5, 1.5))
        y.backward(gos)
        return y

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            if backend == "nccl":
                dist.barrier(device_ids=[dev_index])
            else:
                dist.barrier()
        torch.cuda.synchronize()

    def timed_group(fixed_set=None):
        """EXACTLY --steps steps between barrier + synchronize on both sides; max over ranks.  A HIP event after every step (recorded,
        never waited for inside the group) gives the longest single step of the group: a stall shows up as one long step.  Returns
        (ms per step, longest step, output of the last step); no earlier output is held across steps."""
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
        barrier()
        t0 = time.perf_counter()
        evs[0].record()
        last = None
        for i in range(args.steps):
            if i + 1 < args.steps:
                step(fixed_set)
            else:
                last = step(fixed_set)
            evs[i + 1].record()
        torch.cuda.synchronize()
        barrier()
        dt = time.perf_counter() - t0
        if dist is not None:
            t = torch.tensor([dt], device=dev if backend == "nccl" else "cpu", dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t.item())
        per_step = [evs[i].elapsed_time(evs[i + 1]) for i in range(args.steps)]
        return dt / args.steps * 1e3, max(per_step), last

    # A freshly provisioned box starts with cold clocks / lazily paged-in libraries and memory, and the first touch of every large
    # allocation is paid inside whatever loop makes it (round 3's driver run: one 20-step sample 67 % above the same process's other
    # loops).  Settle, untimed and bounded: groups of 10 steps until THREE consecutive groups agree within 2 % and at least 3 s have
    # passed (at most 15 s).  The timed groups below keep exactly the allocation pattern of these loops (no output is held across steps).
    clocks_before = device_clocks(dev_index) if args.full else None
    t_settle = time.perf_counter()
    settle_groups = []
    agree = 0
    while True:
        tg = time.perf_counter()
        for _ in range(10):
            step()
        torch.cuda.synchronize()
        now = time.perf_counter()
        group = (now - tg) * 100.0  # ms per step
        agree = agree + 1 if settle_groups and abs(group - settle_groups[-1]) <= 0.02 * settle_groups[-1] else 0
        settle_groups.append(group)
        if os.environ.get("BENCH_SETTLE_TRACE"):
            print(f"settle: t={now - t_settle:.2f}s group of 10 steps {group:.3f} ms/step", file=sys.stderr, flush=True)
        if (agree >= 2 and now - t_settle > 3.0) or now - t_settle > 15.0:
            break
    settle = {"groups_of_10_steps": len(settle_groups), "first_ms_per_step": round(settle_groups[0], 4), "last_ms_per_step": round(settle_groups[-1], 4),
              "slowest_ms_per_step": round(max(settle_groups), 4), "elapsed_s": round(time.perf_counter() - t_settle, 2),
              "rule": ">= 3 consecutive groups within 2 % and >= 3 s (cap 15 s)"}
    counter[0] = 0  # the settle ran a varying number of steps: from here on the input set of every step depends on the arguments only

    # ---- the headline: --warmup steps, then ONE group of EXACTLY --steps steps (rotated inputs); ms_per_step = its wall time / --steps ----
    for _ in range(args.warmup):
        step()
    ms_per_step, longest_step_ms, y = timed_group(None)
    y = y.detach()
    xl, Ml, _ = sets[(counter[0] - 1) % n_sets]  # the input set of the last timed step: its .grad is what that step returned
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, {"y": y, "grad_x": xl.grad, "grad_M": Ml.grad})

    full = None
    if args.full:
        # G groups of EXACTLY --steps steps, rotated-input groups (A) interleaved with one-input-set groups (B)
        n_groups = max(1, args.groups)
        rot, one = [], []
        for gi in range(n_groups):
            rot.append(timed_group(None)[:2])
            if n_sets > 1:
                one.append(timed_group(0)[:2])
        clocks_after = device_clocks(dev_index)

        def stats(groups):
            v = sorted(g[0] for g in groups)
            n = len(v)
            med = v[n // 2] if n % 2 else 0.5 * (v[n // 2 - 1] + v[n // 2])
            q = lambda f: v[min(n - 1, max(0, int(round(f * (n - 1)))))]
            return {"median": round(med, 4), "min": round(v[0], 4), "max": round(v[-1], 4), "iqr": round(q(0.75) - q(0.25), 4),
                    "groups": [round(g[0], 4) for g in groups], "longest_single_step_ms": [round(g[1], 3) for g in groups]}

        rot_stats = stats(rot)
        one_stats = stats(one) if one else None
        single_ms = one_stats["median"] if one_stats else None
        full = {
            "ms_per_step_median_of_groups": rot_stats["median"],
            "groups_timing": f"median of {n_groups} groups of {args.steps} steps after the headline, every group bracketed by "
                             "barrier + synchronize (max over ranks); rotated-input groups interleaved with one-input-set groups",
            "ms_per_step_groups": rot_stats["groups"],
            "ms_per_step_min": rot_stats["min"],
            "ms_per_step_max": rot_stats["max"],
            "ms_per_step_iqr": rot_stats["iqr"],
            "longest_single_step_ms_per_group": rot_stats["longest_single_step_ms"],
            "ms_per_step_one_input_set": round(single_ms, 4) if single_ms is not None else None,
            "one_input_set": one_stats,
            "settle": settle,
            "clocks": {"before": clocks_before, "after": clocks_after},
        }

    # ---- optional: the reassembly of the (global_batch, C, S, S) output on every rank, timed on its own ----
    gather = None
    if args.gather != "none" and dist is not None:
        yd = y.detach()
        with torch.no_grad():
            def fwd_only(xs, Ms):
                return K.gaussian_blur2d(K.warp_perspective(xs, Ms, (S, S)), (5, 5), (1.5, 1.5))

            def do():
                if args.gather == "chunked":  # forward of sub-batch i+1 overlapped with the exchange of sub-batch i (forward only)
                    from kornia_amd.distributed import _peer_exchange  # noqa: F401  (documented in kornia_amd/distributed.py)
                    outs = torch.empty(global_batch, C, S, S, device=dev)
                    spans_all = [shard_bounds(global_batch, world, r) for r in range(world)]
                    pend = []
                    for c4 in range(4):
                        spans = []
                        for rlo, rhi in spans_all:
                            clo, chi = shard_bounds(rhi - rlo, 4, c4)
                            spans.append((rlo + clo, rlo + chi))
                        clo, chi = spans[rank]
                        llo = clo - spans_all[rank][0]
                        outs[clo:chi].copy_(fwd_only(x.detach()[llo:llo + (chi - clo)], M.detach()[llo:llo + (chi - clo)]))
                        pend.extend(_peer_exchange(outs, spans, None))
                    for r in pend:
                        r.wait()
                    return outs
                return gather_batch(yd, global_batch, None, "p2p" if args.gather == "p2p" else "all_gather")

            do()
            barrier()
            t1 = time.perf_counter()
            for _ in range(5):
                do()
            barrier()
            gms = (time.perf_counter() - t1) / 5 * 1e3
        gather = {"mode": args.gather, "ms": round(gms, 3), "bytes_received_per_rank": (global_batch - B) * C * S * S * 4,
                  "note": "chunked = forward of 4 sub-batches overlapped with their peer exchange; others = exchange of a finished output"}

    value = global_batch * S * S / (ms_per_step * 1e-3) / 1e6

    if rank == 0:
        result = {
            "metric": "Mpix/s fwd+bwd warp_perspective+GaussianBlur2d Bx3x512x512",
            "value": round(value, 1),
            "unit": "Mpix/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 4),
            "higher_is_better": True,
            "scaling": args.scaling,
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic",
            "config": {
                "workload": f"configs[1]: warp_perspective bilinear + GaussianBlur2d k=5 sigma=1.5, B={B}x{C}x{S}x{S} fp32 fwd+bwd (grad wrt image and homography) per GPU",
                "global_batch": global_batch,
                "parallelism": f"batch-shard x{world} ({args.scaling} scaling), no data-path collective",
            },
            "timing": f"one group of exactly {args.steps} steps after the settle and {args.warmup} warm-up steps, bracketed by barrier + synchronize "
                      "(max over ranks)",
            "longest_single_step_ms": round(longest_step_ms, 3),
            "inputs": f"{n_sets} distinct (x, M, grad_out) sets rotated through the timed loop (a new batch every step)",
        }
        if gather is not None:
            result["gather"] = gather
        if full is not None:
            with torch.no_grad():
                kstats, ops = kernel_roofline(sets, S, max(6, min(args.steps, 21)))
            dom_op = max(ops, key=lambda k: ops[k]["ms"])
            dom_kernel = max(kstats, key=lambda k: kstats[k]["ms"])
            # HBM traffic of the dominant op: rocprofv3 PMC cannot run inside this process, so the figure is the committed measurement of this
            # very command / config (profiles/r0N_pmc_traffic.json: FETCH_SIZE x2 + WRITE_SIZE, separate passes) - quoted only while the
            # kernel sources of the tree hash to what that measurement recorded (csrc_sha256)
            traffic = None
            traffic_note = None
            pmc_doc = json.load(open(PMC_FILE)) if PMC_FILE else {}
            src_now = csrc_sha256()
            if PMC_FILE and pmc_doc.get("csrc_sha256") != src_now:
                # the counters were collected on other kernel sources than the tree's: not this build's traffic
                traffic_note = f"not quoted: profiles/{os.path.basename(PMC_FILE)} was measured on kernel sources {str(pmc_doc.get('csrc_sha256'))[:12]}, the tree is {src_now[:12]}"
            elif (B, C, S) == (256, 3, 512) and PMC_FILE:
                pmc = pmc_doc.get("kernels", {})
                fused = "one read" in ops["km_warp2d_bwd"].get("form", "")
                want = {"km_warp2d_bwd": ("km_warp_bwd_fused_kernel",) if fused else ("km_warp_bwd_tiled_kernel", "km_warp_gm_kernel"), "km_warp2d_fwd": ("km_warp_fwd_box_kernel",),
                        "km_filter2d_sep_fwd": ("km_blur_reg_kernel<float, 5, false",), "km_filter2d_sep_bwd_input": ("km_blur_reg_kernel<float, 5, true",)}[dom_op]
                tot = 0
                for frag in want:
                    hit = [rec["hbm_bytes_per_launch"] for kname, rec in pmc.items() if frag in kname]
                    tot = tot + hit[0] if hit and tot is not None else None
                traffic = tot
            roofline = {
                "bound": "hbm",
                "kernel": {"km_warp2d_bwd": "km_warp2d_bwd (" + ops["km_warp2d_bwd"].get("form", "") + "; dominant launch: " + dom_kernel + ")"}.get(dom_op, dom_op),
                "achieved": ops[dom_op]["GBps"],
                "peak": HBM_PEAK_GBS,
                "unit": "GB/s",
                "frac": ops[dom_op]["frac_of_hbm_peak"],
                "traffic": traffic,
                "traffic_source": (f"profiles/{os.path.basename(PMC_FILE)} (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes, same command; kernel sources {src_now[:12]})"
                                   if traffic else traffic_note),
                "op_ms": ops[dom_op]["ms"],
                "alg_bytes_per_call": ops[dom_op]["alg_bytes"],
                "accounting": "SURVEY.md 8(d): warp fwd 2e, blur fwd 2e, blur bwd 2e, warp bwd 3e bytes per element; op = every launch of the public entry point",
                "dominant_launch": {"name": dom_kernel, **kstats[dom_kernel], "frac_of_hbm_peak": round(kstats[dom_kernel]["GBps"] / HBM_PEAK_GBS, 4)},
            }
            alg_step_bytes = 36 * B * C * S * S
            # the copy bandwidth of THIS box, measured in this process (round 5 printed the literal 6200.0 of round 2's microbenchmark here)
            try:
                copy = measured_streaming_copy(dev)
                best = max(copy["plain"]["GBps_median"], copy["nontemporal"]["GBps_median"])
                roofline["measured_streaming_copy_GBps"] = best
                roofline["measured_streaming_copy"] = copy
                roofline["frac_of_measured_copy"] = round(ops[dom_op]["GBps"] / best, 4)
                step_frac_copy = round(alg_step_bytes / (ms_per_step * 1e-3) / 1e9 / best, 4)
            except Exception as e:  # (informational: never costs the headline)
                roofline["measured_streaming_copy_GBps"] = None
                roofline["measured_streaming_copy"] = {"error": f"{type(e).__name__}: {e}"}
                step_frac_copy = None
            result.update(full)
            result.update({
                "step_GBps_algorithmic": round(alg_step_bytes / (ms_per_step * 1e-3) / 1e9, 1),
                "step_frac_of_hbm_peak": round(alg_step_bytes / (ms_per_step * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                "step_frac_of_measured_copy": step_frac_copy,
                "roofline": roofline,
                "ops": ops,
                "kernels": kstats,
            })
            if world == 1 and not args.no_extras:
                try:
                    result["generic_gpu"] = generic_gpu_baseline(dev, S, C)
                except Exception as e:  # informational only
                    result["generic_gpu"] = {"error": f"{type(e).__name__}: {e}"}
                result["other_configs"] = other_configs(x.device)
            if world == 1 and not args.no_cpu_baseline:
                result["cpu_baseline"] = cpu_baseline(S, C, args.cpu_batch)
            else:
                result["cpu_baseline"] = None
        print(json.dumps(result), flush=True)

    if dist is not None:
        barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
