"""CPU: tests/test_gpu_written_outputs.py - the guarded allocations, the re-exported parity tests and the case table - against the host build
of the shipped kernel sources (the emulated device of tests/test_emulated_kernels.py), entered before the guard."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

if not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):  # pragma: no cover
    pytest.skip("ROCm clang++ (host compiler of the emulated build) not found", allow_module_level=True)

import test_gpu_written_outputs as _w  # noqa: E402

# cases that are about the device itself (tests/test_emulated_kernels.py leaves them out for the same reason)
SKIP = {"test_identity_is_exact_and_errors__warp", "test_half_precision_and_errors__color"}  # both assert that host tensors are refused

for _name in dir(_w):
    if _name.startswith("test_") and callable(getattr(_w, _name)) and _name not in SKIP:
        globals()[f"{_name}__emulated"] = getattr(_w, _name)


@pytest.fixture(autouse=True)
def _emulated_and_guarded(request):
    from mode import emulated_device

    with emulated_device():
        yield from _w.guard_fixture(request)
