"""Masks in the augmentation container on the device: one JSON line.

256x3x224^2 bf16 image with a 256x1x224^2 uint8 (then int64) label mask.  Median over groups of synchronised calls of
  * config 3's pipeline (RandomAffine -> ColorJitter -> RandomGaussianBlur, p = 1) images only, and with the mask;
  * km_warp2d_pair_fwd (image + mask, one matrix) as one launch and as two (image forward + mask kernel), against the image-only masked
    warp and against the composition a user would otherwise write for the mask (cast to bf16, nearest warp, cast back);
  * a RandomPerspective(0.5) pipeline with the mask.
Usage: python profiles/bench_aug_masks.py [--groups 15] [--calls 20]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kornia_amd as K  # noqa: E402
import kornia_amd.augmentation as A  # noqa: E402


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
    B, H, W = 256, 224, 224
    g = torch.Generator().manual_seed(0)
    x = torch.rand(B, 3, H, W, generator=g).to(torch.bfloat16).cuda()
    masks = {"u8": torch.randint(0, 21, (B, 1, H, W), generator=g, dtype=torch.uint8).cuda(),
             "i64": torch.randint(0, 1000, (B, 1, H, W), generator=g).cuda()}
    res = {"shape": [B, 3, H, W], "dtype": "bfloat16", "unit": "ms"}

    def cfg3(keys):
        return A.AugmentationSequential(A.RandomAffine(degrees=15.0, translate=(0.1, 0.1), scale=(0.8, 1.2), shear=5.0, p=1.0),
                                        A.ColorJitter(0.2, 0.2, 0.2, 0.1, p=1.0), A.RandomGaussianBlur((5, 5), (0.1, 2.0), p=1.0), data_keys=keys)

    torch.manual_seed(0)
    img_only = cfg3(["input"])
    res["config3_images"] = timed(lambda: img_only(x), a.groups, a.calls)
    aff = A.RandomAffine(degrees=15.0, translate=(0.1, 0.1), scale=(0.8, 1.2), shear=5.0, p=0.9)
    params = aff.forward_parameters(x.shape)
    p_dev = aff._device_params(params, x.device, False)
    m, M, apply = A.affine_chain(p_dev, x.device, H, W, with_matrix=True)
    from kornia_amd import _native as N
    lib = N.lib()
    res["pair_fused_default"] = lib.km_config_get(b"pair_fused")
    res["image_warp_masked"] = timed(lambda: A.warp_pair(x, masks["u8"][:, :0], m, True, apply=apply), a.groups, a.calls)
    for name, mk in masks.items():
        seq = cfg3(["input", "mask"])
        res[f"config3_with_{name}_mask"] = timed(lambda: seq(x, mk), a.groups, a.calls)
        prev = lib.km_config_set(b"pair_fused", 1)  # km_warp2d_pair_fwd as ONE launch (km_warp_pair_kernel)
        res[f"pair_one_launch_{name}"] = timed(lambda: A.warp_pair(x, mk, m, True, apply=apply), a.groups, a.calls)
        lib.km_config_set(b"pair_fused", 0)  # ... as TWO: the image's own forward, then the mask kernel
        res[f"pair_two_launches_{name}"] = timed(lambda: A.warp_pair(x, mk, m, True, apply=apply), a.groups, a.calls)
        lib.km_config_set(b"pair_fused", prev)
        res[f"mask_composition_{name}"] = timed(lambda: K.warp_affine(mk.to(torch.bfloat16), M[:, :2], (H, W), mode="nearest", align_corners=False).to(mk.dtype),
                                                a.groups, a.calls)
        res[f"mask_bytes_{name}_us_at_5TBps"] = round(2 * mk.numel() * mk.element_size() / 5e12 * 1e6, 1)
    persp = A.AugmentationSequential(A.RandomPerspective(0.5, p=0.8), data_keys=["input", "mask"])
    res["perspective_with_u8_mask"] = timed(lambda: persp(x, masks["u8"]), a.groups, a.calls)
    rp = A.RandomPerspective(0.5, p=0.8)
    pp = rp._device_params(rp.forward_parameters(x.shape), x.device, False)
    mp, _, applyp = A.perspective_chain(pp, x.device, H, W)
    res["perspective_image_warp_masked"] = timed(lambda: A.warp_pair(x, masks["u8"][:, :0], mp, False, apply=applyp), a.groups, a.calls)
    for name, mk in masks.items():
        prev = lib.km_config_set(b"pair_fused", 1)
        res[f"perspective_pair_one_launch_{name}"] = timed(lambda: A.warp_pair(x, mk, mp, False, apply=applyp), a.groups, a.calls)
        lib.km_config_set(b"pair_fused", 0)
        res[f"perspective_pair_two_launches_{name}"] = timed(lambda: A.warp_pair(x, mk, mp, False, apply=applyp), a.groups, a.calls)
        lib.km_config_set(b"pair_fused", prev)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
