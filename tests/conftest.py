import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "snark-verifier-axiom_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs an MI355X (runs through libsvgpu's HIP kernels)")


def load_golden(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def pt(v):
    return None if v is None else (int(v[0], 16), int(v[1], 16))


def q2(v):
    return None if v is None else ((int(v[0][0], 16), int(v[0][1], 16)), (int(v[1][0], 16), int(v[1][1], 16)))


_SANITIZER_PREFIX = None


def sanitizer_prefix():
    """Command prefix for a host binary built with a sanitizer.  The sanitizer runtimes reserve fixed
    address ranges; where the kernel randomises mappings over more bits than the runtime allows for
    (vm.mmap_rnd_bits = 32 against gcc 11's runtimes), a start lands in a reserved range now and
    then and the process dies before main ("unexpected memory mapping").  `setarch -R` turns the
    randomisation off for that one process; where setarch is missing or may not do so, the prefix
    is empty and the binary runs as it is."""
    global _SANITIZER_PREFIX
    if _SANITIZER_PREFIX is None:
        import platform
        import shutil
        import subprocess
        _SANITIZER_PREFIX = []
        setarch = shutil.which("setarch")
        if setarch:
            pre = [setarch, platform.machine(), "-R"]
            try:
                if subprocess.run(pre + ["true"], capture_output=True, timeout=30).returncode == 0:
                    _SANITIZER_PREFIX = pre
            except (OSError, subprocess.TimeoutExpired):
                pass
    return list(_SANITIZER_PREFIX)


@pytest.fixture(scope="session")
def golden_msm():
    return load_golden("msm.json")


@pytest.fixture(scope="session")
def golden_decider():
    return load_golden("decider.json")


@pytest.fixture(scope="session")
def oracle_cpp():
    from oracle import cpu_ref
    if not os.path.exists(cpu_ref.LIB_PATH):
        import subprocess
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle", "cpu")])
    cpu_ref.lib()
    return cpu_ref


@pytest.fixture(scope="session")
def gpu():
    """Initialise libsvgpu on the GPU; fails (never skips) when no GPU is usable."""
    import torch
    import svgpu
    assert torch.cuda.is_available(), "GPU test selected but torch sees no GPU"
    assert svgpu.init() >= 1
    return torch.device("cuda:0")
