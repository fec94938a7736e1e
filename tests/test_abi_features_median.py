"""CPU: km_median_blur_supported / _fwd / _bwd are announced by bit 2 of km_abi_features() (include/kornia_amd.h, Versioning), exported by the
library and declared in the header, while the ABI version stays 3."""
import ctypes
import os
import re

from kornia_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("km_median_blur_supported", "km_median_blur_fwd", "km_median_blur_bwd")


def test_features_bit2_and_version_3():
    from kornia_amd import build

    lib = ctypes.CDLL(build.build())
    lib.km_abi_features.restype = ctypes.c_int
    lib.km_abi_version.restype = ctypes.c_int
    assert lib.km_abi_features() & 4 and _native.ABI_FEATURES & 4
    assert lib.km_abi_features() & 3 == 3  # the earlier groups are still announced
    assert lib.km_abi_version() == _native.ABI_VERSION == 3
    for name in SYMBOLS:
        assert hasattr(lib, name) and _native._FEATURE_SYMBOLS[name] == 4
    # the window and dtype query needs no device: odd sides of 1 .. 15, the four dtypes
    lib.km_median_blur_supported.argtypes = [ctypes.c_int] * 3
    assert all(lib.km_median_blur_supported(ky, kx, dt) == 1 for ky, kx in ((1, 1), (3, 3), (5, 1), (9, 3), (15, 15)) for dt in range(4))
    assert not any(lib.km_median_blur_supported(ky, kx, dt) for ky, kx, dt in ((17, 17, 0), (3, 17, 0), (4, 4, 0), (3, 2, 2), (0, 3, 0), (3, 3, 4)))


def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "kornia_amd.h")).read()
    declared = set(re.findall(r"^(?:int|const char\*|long long)\s+(km_\w+)\(", text, flags=re.M))
    assert set(SYMBOLS) <= declared and set(SYMBOLS) <= set(_native.exported_symbols())
    assert re.search(r"bit 2\s+km_median_blur_supported, km_median_blur_fwd, km_median_blur_bwd", text)
    assert "currently 3" in text
