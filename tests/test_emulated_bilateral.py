"""CPU: tests/test_gpu_bilateral.py, unchanged, against the host build of the shipped kernel sources (the emulated device of
tests/test_emulated_kernels.py)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):  # pragma: no cover
    pytest.skip("ROCm clang++ (host compiler of the emulated build) not found", allow_module_level=True)

import test_gpu_bilateral as _m  # noqa: E402

for _name in dir(_m):
    if _name.startswith("test_") and callable(getattr(_m, _name)):
        globals()[f"{_name}__emulated"] = getattr(_m, _name)


@pytest.fixture(autouse=True)
def _emulated():
    from mode import emulated_device

    with emulated_device():
        yield
