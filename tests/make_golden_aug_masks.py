"""Generates tests/golden/aug_masks.npz from the reference (Kornia) - run in a checkout next to the reference tree, not by the suite:

    python tests/make_golden_aug_masks.py

``torch.manual_seed(s)`` followed by ``AugmentationSequential(..., data_keys=["input", "mask", ...])(x, masks...)`` and ``aug.inverse(...)`` of
what it returned: the parameters Kornia draws, the head of the generator state afterwards, the outputs and the inverses, for
tests/test_gpu_aug_masks.py (which compares kornia_amd.augmentation's container against them on a machine without Kornia)."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def pipelines(K):
    from kornia.augmentation import AugmentationSequential, ColorJitter, RandomAffine, RandomGaussianBlur, RandomPerspective

    return {
        # i. BASELINE config 3 with a uint8 label mask
        "config3": (lambda: AugmentationSequential(RandomAffine(degrees=15.0, translate=(0.1, 0.1), scale=(0.8, 1.2), shear=5.0, p=1.0),
                                                   ColorJitter(0.2, 0.2, 0.2, 0.1, p=1.0), RandomGaussianBlur((5, 5), (0.1, 2.0), p=1.0),
                                                   data_keys=["input", "mask"]), torch.float32, ("u8",), ["input", "mask"]),
        # ii. perspective + affine with border padding, bf16 image, int64 labels up to 1000
        "persp_border": (lambda: AugmentationSequential(RandomPerspective(0.4, p=0.6),
                                                        RandomAffine(degrees=20.0, translate=(0.1, 0.1), scale=(0.9, 1.1), padding_mode="border", p=0.7),
                                                        data_keys=["input", "mask"]), torch.bfloat16, ("i64",), ["input", "mask"]),
        # iii. area-preserving perspective + affine with a fill value, same_on_batch, a bool mask and a 2-channel float32 mask
        "area_fill": (lambda: AugmentationSequential(RandomPerspective(0.5, sampling_method="area_preserving", p=0.8),
                                                     RandomAffine(degrees=25.0, shear=(-5.0, 5.0), padding_mode="fill", fill_value=0.3, p=0.7),
                                                     data_keys=["input", "mask", "mask"], same_on_batch=True), torch.float32, ("bool", "f32x2"),
                      ["input", "mask", "mask"]),
    }


def masks(kinds, g):
    out = []
    for k in kinds:
        if k == "u8":
            out.append(torch.randint(0, 21, (5, 1, 40, 56), generator=g, dtype=torch.uint8))
        elif k == "i64":
            out.append(torch.randint(0, 1001, (5, 1, 40, 56), generator=g, dtype=torch.int64))
        elif k == "bool":
            out.append(torch.rand(5, 1, 40, 56, generator=g) > 0.5)
        else:
            out.append(torch.randint(0, 9, (5, 2, 40, 56), generator=g).float() / 8)  # (soft labels in eighths)
    return out


def main() -> None:
    from ref_shim import import_reference

    K = import_reference()
    g = torch.Generator().manual_seed(909)
    d = {"x": torch.rand(5, 3, 40, 56, generator=g)}
    for pname, (make, dt, kinds, keys) in pipelines(K).items():
        ms = masks(kinds, g)
        for i, mk in enumerate(ms):
            d[f"{pname}__mask{i}"] = mk
        for seed in (3, 11):
            if dt != torch.float32:
                # a 16-bit pipeline is ALSO run on the float32 image with the same seed (the draws are float32 either way): Kornia casts its
                # matrices to the image dtype (`.to(input)`) and warps with 16-bit homographies, which kornia_amd does not do (its matrices stay
                # float32), so the outputs are recorded from the float32 run - the test compares the 16-bit result against them within the
                # 16-bit bounds - and the 16-bit run contributes its parameters and generator state
                torch.manual_seed(seed)
                aug32 = make()
                it = iter(ms)
                outs32 = aug32(*[d["x"] if k == "input" else next(it) for k in keys])
                rng32 = torch.get_rng_state()[:64].clone()
                inv32 = aug32.inverse(*outs32)
            torch.manual_seed(seed)
            aug = make()
            it = iter(ms)
            args = [d["x"].to(dt) if k == "input" else next(it) for k in keys]
            outs = aug(*args)
            key = f"{pname}__seed{seed}"
            d[key + "__rng_after"] = torch.get_rng_state()[:64].clone()
            for item in aug._params:
                for k, v in item.data.items():
                    if isinstance(v, torch.Tensor):
                        d[f"{key}__{item.name}__{k}"] = v
            inv = aug.inverse(*outs)
            if dt != torch.float32:
                assert torch.equal(rng32, d[key + "__rng_after"])
                for it32, item in zip(aug32._params, aug._params):
                    for k, v in item.data.items():
                        assert not isinstance(v, torch.Tensor) or torch.equal(v, it32.data[k]), k
                outs, inv = outs32, inv32
            j = 0
            for k, o, v in zip(keys, outs, inv):
                name = "out" if k == "input" else f"mask{j}"
                j += k == "mask"
                # (size: the float32 outputs of a 16-bit pipeline and every inverse image in float16 - the bounds they meet are wider than its
                # rounding - the inverse image for the first seed only)
                d[f"{key}__{name}"] = o.to(torch.float16) if (k == "input" and dt != torch.float32) else o
                if k != "input":
                    d[f"{key}__inv_{name}"] = v
                elif seed == 3:
                    d[f"{key}__inv_{name}"] = v.to(torch.float16)
    arrays = {k: v.contiguous().numpy() for k, v in d.items()}
    path = os.path.join(ROOT, "tests", "golden", "aug_masks.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    torch.set_num_threads(4)
    main()
