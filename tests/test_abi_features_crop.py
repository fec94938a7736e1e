"""CPU: km_crop_resize_fwd is announced by bit 1 of km_abi_features() (include/kornia_amd.h, Versioning), exported by the library and
declared in the header, while the ABI version stays 3."""
import ctypes
import os
import re

from kornia_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_features_bit1_and_version_3():
    from kornia_amd import build

    lib = ctypes.CDLL(build.build())
    lib.km_abi_features.restype = ctypes.c_int
    lib.km_abi_version.restype = ctypes.c_int
    assert lib.km_abi_features() & 2 and _native.ABI_FEATURES & 2
    assert lib.km_abi_version() == _native.ABI_VERSION == 3
    assert hasattr(lib, "km_crop_resize_fwd")
    assert _native._FEATURE_SYMBOLS["km_crop_resize_fwd"] == 2


def test_header_declares_the_entry_point():
    text = open(os.path.join(ROOT, "include", "kornia_amd.h")).read()
    declared = set(re.findall(r"^(?:int|const char\*|long long)\s+(km_\w+)\(", text, flags=re.M))
    assert "km_crop_resize_fwd" in declared and "km_crop_resize_fwd" in _native.exported_symbols()
    assert re.search(r"bit 1\s+km_crop_resize_fwd", text)
