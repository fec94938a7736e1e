"""CPU: the entry points added after ABI set 3 are announced by km_abi_features() (include/kornia_amd.h, Versioning) while the version stays 3,
and the header and the binding still declare the same symbols."""
import ctypes
import os
import re

from kornia_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_features_bit0_and_version_3():
    from kornia_amd import build

    lib = ctypes.CDLL(build.build())
    lib.km_abi_features.restype = ctypes.c_int
    lib.km_abi_version.restype = ctypes.c_int
    assert lib.km_abi_features() & 1 and _native.ABI_FEATURES & 1
    assert lib.km_abi_version() == _native.ABI_VERSION == 3
    for name in ("km_warp2d_pair_fwd", "km_perspective_params_chain_fwd", "km_inverse_chain_fwd", "km_abi_features"):
        assert hasattr(lib, name), name


def test_header_and_binding_list_the_same_symbols():
    text = open(os.path.join(ROOT, "include", "kornia_amd.h")).read()
    declared = sorted(set(re.findall(r"^(?:int|const char\*|long long)\s+(km_\w+)\(", text, flags=re.M)))
    assert sorted(_native.exported_symbols()) == declared
    assert {"km_warp2d_pair_fwd", "km_perspective_params_chain_fwd", "km_inverse_chain_fwd", "km_abi_features"} <= set(declared)
