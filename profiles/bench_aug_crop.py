"""RandomResizedCrop and the random flips on the device: one JSON line.

256x3x256^2 -> 224^2, in bfloat16 and in float32.  Median over groups of synchronised calls of
  * km_crop_resize_fwd on one draw of RandomResizedCrop(224) (image only), with its GB/s on the algorithmic bytes: the rows of the drawn
    windows read ONCE (a window's rows are those its resize touches: all of them) plus B*C*224^2 written;
  * the container call RandomResizedCrop(224) -> RandomHorizontalFlip -> ColorJitter, images only and with a uint8 label mask;
  * for comparison, on the same device and draw: the per-sample composition of the package's own ops (slice -> resize_bilinear ->
    torch.flip / select_samples) and Kornia's algorithm restated in torch (one .tolist() of the boxes, slice + F.interpolate per sample,
    torch.flip + torch.where).
Usage: python profiles/bench_aug_crop.py [--groups 15] [--calls 20]"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kornia_amd.augmentation as A  # noqa: E402
from kornia_amd.geometry.transform import resize_bilinear  # noqa: E402
from kornia_amd.geometry.transform.crop2d import crop_resize  # noqa: E402


def timed(fn, groups, calls):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=15)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    B, C, H, W, S = 256, 3, 256, 256, 224
    g = torch.Generator().manual_seed(0)
    x32 = torch.rand(B, C, H, W, generator=g)
    mk = torch.randint(0, 21, (B, 1, H, W), generator=g, dtype=torch.uint8).cuda()
    res = {"shape": [B, C, H, W], "size": [S, S], "unit": "ms"}
    torch.manual_seed(0)
    rrc = A.RandomResizedCrop((S, S))
    params = rrc.forward_parameters((B, C, H, W))
    src_h = params["src"].clone()
    src = src_h.cuda()
    s = src_h.to(torch.long)
    rows = ((s[:, 3, 1] + 1 - s[:, 0, 1]) * (s[:, 1, 0] + 1 - s[:, 0, 0])).sum().item()  # window pixels per channel, summed over the batch
    flip = (torch.rand(B) < 0.5).float()
    flip_d = flip.cuda()
    for name, dt in (("bf16", torch.bfloat16), ("f32", torch.float32)):
        x = x32.to(dt).cuda()
        esz = x.element_size()
        nbytes = (rows * C + B * C * S * S) * esz
        t = timed(lambda: crop_resize(x, None, src, (S, S)), a.groups, a.calls)
        res[f"{name}_kernel_ms"] = t
        res[f"{name}_kernel_GBps"] = round(nbytes / (t * 1e-3) / 1e9, 1)
        res[f"{name}_kernel_bytes"] = int(nbytes)
        t = timed(lambda: crop_resize(x, mk, src, (S, S), flip_x=flip_d), a.groups, a.calls)
        res[f"{name}_kernel_with_u8_mask_and_flip_ms"] = t

        torch.manual_seed(0)
        seq = A.AugmentationSequential(A.RandomResizedCrop((S, S)), A.RandomHorizontalFlip(), A.ColorJitter(0.2, 0.2, 0.2, 0.1, p=1.0))
        res[f"{name}_container_images_ms"] = timed(lambda: seq(x), a.groups, a.calls)
        seqm = A.AugmentationSequential(A.RandomResizedCrop((S, S)), A.RandomHorizontalFlip(), A.ColorJitter(0.2, 0.2, 0.2, 0.1, p=1.0),
                                        data_keys=["input", "mask"])
        res[f"{name}_container_with_u8_mask_ms"] = timed(lambda: seqm(x, mk), a.groups, a.calls)

        def package_loop():
            sl = s.tolist()
            out = torch.cat([resize_bilinear(x[i:i + 1, :, sl[i][0][1]:sl[i][3][1] + 1, sl[i][0][0]:sl[i][1][0] + 1], (S, S), True) for i in range(B)])
            return A.select_samples(out.flip(-1), out, flip_d > 0.5)

        def kornia_restated():
            bx = src.long()  # (Kornia's crop_by_indices: the boxes as long on the device, one .tolist())
            x1, x2, y1, y2 = torch.stack([bx[:, 0, 0], bx[:, 1, 0] + 1, bx[:, 0, 1], bx[:, 3, 1] + 1]).tolist()
            out = torch.empty(B, C, S, S, device=x.device, dtype=x.dtype)
            for i in range(B):
                w = x[i:i + 1, :, y1[i]:y2[i], x1[i]:x2[i]]
                out[i] = F.interpolate(w, size=(S, S), mode="bilinear", align_corners=True) if w.shape[-2:] != (S, S) else w
            return torch.where((flip_d > 0.5).view(-1, 1, 1, 1), out.flip(-1), out)

        res[f"{name}_package_per_sample_loop_ms"] = timed(package_loop, max(3, a.groups // 3), max(2, a.calls // 5))
        res[f"{name}_kornia_restated_ms"] = timed(kornia_restated, max(3, a.groups // 3), max(2, a.calls // 5))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
