"""CPU: km_bilateral_blur_fwd / _bwd are announced by bit 3 of km_abi_features() (include/kornia_amd.h, Versioning), exported by the library and
declared in the header, while the ABI version stays 3 and bits 0-2 stay set."""
import ctypes
import os
import re

from kornia_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("km_bilateral_blur_fwd", "km_bilateral_blur_bwd")


def test_features_bit3_and_version_3():
    from kornia_amd import build

    lib = ctypes.CDLL(build.build())
    lib.km_abi_features.restype = ctypes.c_int
    lib.km_abi_version.restype = ctypes.c_int
    assert lib.km_abi_features() & 8 and _native.ABI_FEATURES & 8
    assert lib.km_abi_features() & 7 == 7 and _native.ABI_FEATURES == 15  # the earlier groups are still announced
    assert lib.km_abi_version() == _native.ABI_VERSION == 3
    for name in SYMBOLS:
        assert hasattr(lib, name) and _native._FEATURE_SYMBOLS[name] == 8
    assert not hasattr(lib, "km_bilateral_blur_supported")  # (no query symbol: the limits are the header's, the predicate is Python's)
    # the argument checks need no device: an even or oversized window, too many channels, a reflect pad that does not fit
    lib.km_last_error.restype = ctypes.c_char_p
    fwd = lib.km_bilateral_blur_fwd
    fwd.argtypes = _native._PROTOTYPES["km_bilateral_blur_fwd"]
    fwd.restype = ctypes.c_int

    def call(C=1, H=8, W=8, ky=3, kx=3, border=0):
        return fwd(None, None, None, None, None, None, 1, C, C, H, W, 1, 1, ky, kx, border, 0, 0, None)

    for kw, word in ((dict(ky=4), "odd"), (dict(ky=17, kx=17), "odd"), (dict(C=17), "channels"), (dict(border=1, ky=5, kx=5, H=2), "reflect")):
        assert call(**kw) < 0 and word in lib.km_last_error().decode(), kw
    assert call(H=0) == 0  # an empty image: nothing to launch


def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "kornia_amd.h")).read()
    declared = set(re.findall(r"^(?:int|const char\*|long long)\s+(km_\w+)\(", text, flags=re.M))
    assert set(SYMBOLS) <= declared and set(SYMBOLS) <= set(_native.exported_symbols())
    assert re.search(r"bit 3\s+km_bilateral_blur_fwd, km_bilateral_blur_bwd", text)
    assert "currently 3" in text and "KM_DIST_L1 = 0, KM_DIST_L2 = 1" in text
    assert len(_native._PROTOTYPES["km_bilateral_blur_fwd"]) == 19 and len(_native._PROTOTYPES["km_bilateral_blur_bwd"]) == 22
