"""Build-container only (needs the reference tree): under kornia_amd.patch() ``kornia.filters.bilateral_blur`` and ``joint_bilateral_blur`` on
"device" tensors (the host build of the kernels, tests/emu) reach km_bilateral_blur_fwd and return what the unpatched reference returns on the
CPU within the fp32 bound; the gradient flows through the native backward; a window the native op refuses and a CPU tensor fall through to
Kornia's function with no native call; unpatch() restores the originals."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import ref_shim  # noqa: E402

pytestmark = pytest.mark.skipif(not ref_shim.reference_available(), reason="reference tree not present (GPU box)")

F32_BOUND = 1e-5   # tests/test_gpu_bilateral.py
GRAD_BOUND = 1e-5  # of the largest entry


def test_bilateral_blur_under_patch_on_the_host_build():
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("host build of the kernels needs ROCm's clang++")
    K = ref_shim.import_reference()
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
    import kornia.filters.bilateral as bil_mod
    from mode import emulated_device

    import kornia_amd.kornia_patch as P

    orig, orig_joint = bil_mod.bilateral_blur, bil_mod.joint_bilateral_blur
    gen = torch.Generator().manual_seed(3)
    x, g = torch.rand(2, 3, 20, 24, generator=gen), torch.rand(2, 1, 20, 24, generator=gen)
    ss = (1.5, 1.1)
    refs = {k: orig(x, k, 0.1, ss) for k in ((3, 3), (5, 5), (3, 7), (17, 17))}
    ref_kw = orig(x, kernel_size=5, sigma_color=0.5, sigma_space=ss, border_type="replicate", color_distance_type="l2")
    ref_joint = orig_joint(x, g, (5, 5), 0.1, ss)
    ref_ts = orig(x, (5, 5), torch.tensor([0.2, 0.6]), torch.tensor([[1.5, 1.1], [0.8, 2.0]]))
    xr, gr = x.clone().requires_grad_(), g.clone().requires_grad_()
    orig_joint(xr, gr, (3, 3), 0.5, ss).square().sum().backward()
    sg = torch.tensor([0.5], requires_grad=True)
    ref_sg = orig(x, (3, 3), sg, ss)

    with emulated_device():
        import emu_lib

        calls, bwd_calls = [], []
        real, real_bwd = emu_lib.lib().km_bilateral_blur_fwd, emu_lib.lib().km_bilateral_blur_bwd

        n = P.patch()
        try:
            assert bil_mod.bilateral_blur.__wrapped__ is orig and bil_mod.joint_bilateral_blur.__wrapped__ is orig_joint
            assert K.filters.bilateral_blur is bil_mod.bilateral_blur and K.filters.joint_bilateral_blur is bil_mod.joint_bilateral_blur

            def counted(*a):
                calls.append((a[1] is not None, a[13], a[14]))  # (joint, ky, kx)
                return real(*a)

            def counted_bwd(*a):
                bwd_calls.append((a[16], a[17]))
                return real_bwd(*a)

            from kornia_amd import _native as N

            N.lib().km_bilateral_blur_fwd = counted
            N.lib().km_bilateral_blur_bwd = counted_bwd
            try:
                for k in ((3, 3), (5, 5), (3, 7)):
                    assert (K.filters.bilateral_blur(x.cuda(), k, 0.1, ss) - refs[k]).abs().max().item() <= F32_BOUND, k
                out = K.filters.bilateral_blur(x.cuda(), kernel_size=5, sigma_color=0.5, sigma_space=ss, border_type="replicate", color_distance_type="l2")
                assert (out - ref_kw).abs().max().item() <= F32_BOUND
                assert (K.filters.joint_bilateral_blur(x.cuda(), g.cuda(), (5, 5), 0.1, ss) - ref_joint).abs().max().item() <= F32_BOUND
                out = K.filters.bilateral_blur(x.cuda(), (5, 5), torch.tensor([0.2, 0.6]).cuda(), torch.tensor([[1.5, 1.1], [0.8, 2.0]]).cuda())
                assert (out - ref_ts).abs().max().item() <= F32_BOUND
                assert calls == [(False, 3, 3), (False, 5, 5), (False, 3, 7), (False, 5, 5), (True, 5, 5), (False, 5, 5)]
                # the modules call the functions of their own module: native too
                assert (K.filters.BilateralBlur((3, 3), 0.1, ss)(x.cuda()) - refs[(3, 3)]).abs().max().item() <= F32_BOUND and len(calls) == 7
                # the gradient flows through the native backward
                xg, gg = x.cuda().requires_grad_(), g.cuda().requires_grad_()
                K.filters.joint_bilateral_blur(xg, gg, (3, 3), 0.5, ss).square().sum().backward()
                assert bwd_calls == [(3, 3)] and len(calls) == 8
                for got, ref in ((xg.grad, xr.grad), (gg.grad, gr.grad)):
                    assert (got - ref).abs().max().item() <= GRAD_BOUND * ref.abs().max().item()
                # what the native op refuses: Kornia's own function, no native call, no error
                assert torch.equal(K.filters.bilateral_blur(x.cuda(), (17, 17), 0.1, ss), refs[(17, 17)]) and len(calls) == 8
                sgd = torch.tensor([0.5]).cuda().requires_grad_()
                out = K.filters.bilateral_blur(x.cuda(), (3, 3), sgd, ss)  # a sigma that needs a gradient
                assert torch.equal(out, ref_sg) and out.requires_grad and len(calls) == 8
                # even sizes and a bad distance name keep Kornia's own errors
                with pytest.raises(RuntimeError):
                    K.filters.bilateral_blur(x.cuda(), (4, 4), 0.1, ss)
                with pytest.raises(ValueError, match="color_distance_type only accepts l1 or l2"):
                    K.filters.bilateral_blur(x.cuda(), (3, 3), 0.1, ss, "reflect", "l3")
                assert len(calls) == 8
            finally:
                N.lib().km_bilateral_blur_fwd = real
                N.lib().km_bilateral_blur_bwd = real_bwd
        finally:
            assert P.unpatch() == n
    assert bil_mod.bilateral_blur is orig and bil_mod.joint_bilateral_blur is orig_joint and K.filters.bilateral_blur is orig and not P.is_patched()
    assert K.filters.joint_bilateral_blur is orig_joint


def test_cpu_tensors_fall_through():
    """outside the emulated device a CPU tensor is no device tensor: the dispatcher hands it to Kornia's function, the native library is not touched"""
    K = ref_shim.import_reference()
    import kornia.filters.bilateral as bil_mod

    import kornia_amd.kornia_patch as P
    from kornia_amd import _native as N

    orig = bil_mod.bilateral_blur
    x = torch.rand(1, 3, 12, 14, generator=torch.Generator().manual_seed(5))
    ref = orig(x, (3, 3), 0.1, (1.5, 1.5))
    real_lib = N.lib

    def no_lib():
        raise AssertionError("the native library was asked for a CPU tensor")

    n = P.patch()
    try:
        N.lib = no_lib
        assert torch.equal(K.filters.bilateral_blur(x, (3, 3), 0.1, (1.5, 1.5)), ref)
        assert torch.equal(K.filters.joint_bilateral_blur(x, x, (3, 3), 0.1, (1.5, 1.5)), ref)
    finally:
        N.lib = real_lib
        assert P.unpatch() == n
    assert bil_mod.bilateral_blur is orig
