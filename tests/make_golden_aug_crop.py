"""Generates tests/golden/aug_crop.npz from the reference (Kornia) - run in a checkout next to the reference tree, not by the suite:

    python tests/make_golden_aug_crop.py

``torch.manual_seed(s)`` followed by pipelines of ``RandomResizedCrop`` and the random flips (with ``ColorJitter`` / ``RandomAffine``) and a
label mask: the parameters Kornia draws, the head of the generator state afterwards, the outputs and, where Kornia allows it, the inverses;
and a few direct ``kornia.geometry.transform.crop_by_indices`` calls - for tests/test_gpu_aug_crop.py, which compares kornia_amd against
them on a machine without Kornia."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def pipelines():
    from kornia.augmentation import AugmentationSequential, ColorJitter, RandomAffine, RandomHorizontalFlip, RandomResizedCrop, RandomVerticalFlip

    return {
        # i. the ImageNet recipe with a uint8 label mask
        "rrc_hflip_jitter": (lambda: AugmentationSequential(RandomResizedCrop((24, 32)), RandomHorizontalFlip(), ColorJitter(0.2, 0.2, 0.2, 0.1, p=1.0),
                                                            data_keys=["input", "mask"]), torch.float32, "u8", False),
        # ii. wider scale / ratio ranges, one box for the batch, a vertical flip; bf16 image, int64 labels up to 1000
        "rrc_same_vflip": (lambda: AugmentationSequential(RandomResizedCrop((24, 32), scale=(0.3, 1.0), ratio=(0.5, 2.0), same_on_batch=True),
                                                          RandomVerticalFlip(p=0.7), data_keys=["input", "mask"]), torch.bfloat16, "i64", False),
        # iii. resample-mode crop, then an affine that samples at the crop's size (centre (15.5, 11.5)); inverse back to the input size
        "rrc_resample_affine": (lambda: AugmentationSequential(RandomResizedCrop((24, 32), cropping_mode="resample"),
                                                               RandomAffine(degrees=20.0, translate=(0.1, 0.1), scale=(0.9, 1.1), p=0.7),
                                                               data_keys=["input", "mask"]), torch.float32, "u8", True),
        # iv. flips alone, inverse
        "flips": (lambda: AugmentationSequential(RandomHorizontalFlip(), RandomVerticalFlip(p=0.5), data_keys=["input", "mask"]), torch.float32,
                  "bool", True),
    }


def make_mask(kind, g):
    if kind == "u8":
        return torch.randint(0, 21, (5, 1, 40, 56), generator=g, dtype=torch.uint8)
    if kind == "i64":
        return torch.randint(0, 1001, (5, 1, 40, 56), generator=g, dtype=torch.int64)
    return torch.rand(5, 1, 40, 56, generator=g) > 0.5


def crop_cases(g):
    """(name, boxes, kwargs) of the direct crop_by_indices calls."""
    def box(x0, y0, w, h):
        return [[x0, y0], [x0 + w - 1, y0], [x0 + w - 1, y0 + h - 1], [x0, y0 + h - 1]]

    per_sample = torch.tensor([box(3, 2, 20, 15), box(0, 0, 56, 40), box(30, 10, 9, 7), box(10, 25, 12, 15), box(5, 5, 12, 16)], dtype=torch.float32)
    same = torch.tensor([box(7, 4, 22, 18)] * 5, dtype=torch.float32)
    equal = torch.tensor([box(1, 2, 16, 12), box(40, 28, 16, 12), box(0, 0, 16, 12), box(20, 9, 16, 12), box(33, 1, 16, 12)], dtype=torch.float32)
    return [
        ("boxes", per_sample, dict(size=(12, 16))),
        ("boxes_ac_true", per_sample, dict(size=(12, 16), align_corners=True)),
        ("boxes_ac_false", per_sample, dict(size=(12, 16), align_corners=False)),
        ("same_pad", same, dict(size=(12, 16), shape_compensation="pad")),
        ("equal", equal, dict(size=(12, 16))),
        ("pad", per_sample, dict(size=(12, 16), shape_compensation="pad")),
        ("size_none", equal, dict()),
        ("nearest", per_sample, dict(size=(12, 16), interpolation="nearest")),
    ]


def main() -> None:
    from ref_shim import import_reference

    K = import_reference()
    g = torch.Generator().manual_seed(707)
    d = {"x": torch.rand(5, 3, 40, 56, generator=g)}
    for pname, (make, dt, kind, inverse) in pipelines().items():
        mk = make_mask(kind, g)
        d[f"{pname}__mask"] = mk
        for seed in (3, 11):
            if dt != torch.float32:
                # (a 16-bit pipeline is ALSO run on the float32 image: the outputs are recorded from that run, the 16-bit run contributes its
                # parameters and generator state, which are the same - as tests/make_golden_aug_masks.py does)
                torch.manual_seed(seed)
                aug32 = make()
                out32 = aug32(d["x"], mk)
                rng32 = torch.get_rng_state()[:64].clone()
            torch.manual_seed(seed)
            aug = make()
            outs = aug(d["x"].to(dt), mk)
            key = f"{pname}__seed{seed}"
            d[key + "__rng_after"] = torch.get_rng_state()[:64].clone()
            for item in aug._params:
                for k, v in item.data.items():
                    if isinstance(v, torch.Tensor):
                        d[f"{key}__{item.name}__{k}"] = v
            if dt != torch.float32:
                assert torch.equal(rng32, d[key + "__rng_after"])
                for it32, item in zip(aug32._params, aug._params):
                    for k, v in item.data.items():
                        assert not isinstance(v, torch.Tensor) or torch.equal(v, it32.data[k]), k
                outs = out32
            if pname == "flips":
                continue  # (a flip is exact: the test rebuilds Kornia's output from the parameters and x)
            d[key + "__out"] = outs[0].to(torch.float16) if dt != torch.float32 else outs[0]
            d[key + "__mask_out"] = outs[1]
            if inverse:
                inv = aug.inverse(*outs)
                d[key + "__inv_mask"] = inv[1]
                if seed == 3:
                    d[key + "__inv_out"] = inv[0].to(torch.float16)
    from kornia.geometry.transform import crop_by_indices

    for name, boxes, kw in crop_cases(g):
        d[f"cbi__{name}__boxes"] = boxes
        d[f"cbi__{name}__out"] = crop_by_indices(d["x"], boxes, **kw)
    arrays = {k: v.contiguous().numpy() for k, v in d.items()}
    path = os.path.join(ROOT, "tests", "golden", "aug_crop.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    torch.set_num_threads(4)
    main()
