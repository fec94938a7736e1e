"""Build-container only (needs the reference tree): under kornia_amd.patch() ``kornia.filters.median_blur`` and Kornia's own ``RandomMedianBlur`` on
"device" tensors (the host build of the kernels, tests/emu) reach km_median_blur_fwd and return what the unpatched reference returns on the CPU; a
window the native op refuses falls through to Kornia's function; unpatch() restores the original."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import ref_shim  # noqa: E402

pytestmark = pytest.mark.skipif(not ref_shim.reference_available(), reason="reference tree not present (GPU box)")


def test_median_blur_under_patch_on_the_host_build():
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("host build of the kernels needs ROCm's clang++")
    K = ref_shim.import_reference()
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
    import kornia.augmentation._2d.intensity.median_blur as rmb_mod
    import kornia.filters.median as med_mod
    from mode import emulated_device

    import kornia_amd.kornia_patch as P

    orig = med_mod.median_blur
    x = torch.rand(5, 3, 20, 24, generator=torch.Generator().manual_seed(3))
    refs = {k: orig(x, k) for k in ((3, 3), (5, 5), (3, 7), (17, 17))}
    ref16 = orig(x.bfloat16(), (5, 5))
    torch.manual_seed(11)
    aug = K.augmentation.RandomMedianBlur((3, 3), p=0.5)
    ref_aug = aug(x)
    params = aug._params
    on = torch.as_tensor(params["batch_prob"]) > 0.5
    assert 0 < int(on.sum()) < 5, "the draw must mix transformed and untouched samples"
    xr = x.clone().requires_grad_()
    orig(xr, (3, 3)).sum().backward()

    with emulated_device():
        import emu_lib

        calls = []
        real = emu_lib.lib().km_median_blur_fwd

        n = P.patch()
        try:
            assert med_mod.median_blur.__wrapped__ is orig and K.filters.median_blur is med_mod.median_blur
            assert rmb_mod.median_blur is med_mod.median_blur  # the by-value import of the augmentation module is rebound too

            def counted(*a):
                calls.append(a[8:10])  # (ky, kx)
                return real(*a)

            from kornia_amd import _native as N

            N.lib().km_median_blur_fwd = counted
            try:
                for k in ((3, 3), (5, 5), (3, 7)):
                    assert torch.equal(K.filters.median_blur(x.cuda(), k), refs[k]), k
                assert torch.equal(K.filters.median_blur(x.bfloat16().cuda(), (5, 5)), ref16)
                assert calls == [(3, 3), (5, 5), (3, 7), (5, 5)]
                # a window the native op refuses: Kornia's own function, no native call, no error
                assert torch.equal(K.filters.median_blur(x.cuda(), (17, 17)), refs[(17, 17)]) and len(calls) == 4
                # even sizes keep Kornia's own error
                with pytest.raises(RuntimeError):
                    K.filters.median_blur(x.cuda(), (4, 4))
                assert len(calls) == 4
                # Kornia's module with its own sampled parameters replayed on "device" tensors
                out = aug(x.cuda(), params=params)
                assert calls[4:] == [(3, 3)] and torch.equal(out, ref_aug)
                # the gradient flows through the native backward
                xg = x.cuda().requires_grad_()
                K.filters.median_blur(xg, (3, 3)).sum().backward()
                assert torch.equal(xg.grad, xr.grad)
            finally:
                N.lib().km_median_blur_fwd = real
            # CPU tensors keep flowing to Kornia's own code
        finally:
            assert P.unpatch() == n
    assert med_mod.median_blur is orig and K.filters.median_blur is orig and rmb_mod.median_blur is orig and not P.is_patched()
