"""The weight packs on the CPU: tools/pack_digest.cpp (csrc/pack.cpp alone, no device) against the
digests recorded from the pack functions as they stood in runtime.cpp (golden/pack_digests.txt,
profiles/packs/README.md).  A wrong index or rounding in any layout changes its line."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "isl-signlanguage-translation_amd", "csrc")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _host_compiler():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for c in (os.path.join(rocm, "llvm", "bin", "clang++"), shutil.which("amdclang++")):
        if c and os.path.exists(c):
            return c
    return None


# the development build adds the wino_x3 pack; the product build prints every other line
@pytest.mark.parametrize("dev", [False, True], ids=["product", "dev"])
def test_pack_digests(tmp_path, dev):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no ROCm host compiler")
    exe = str(tmp_path / "pack_digest")
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-I" + CSRC]
                   + (["-DISLPOSE_DEV"] if dev else [])
                   + [os.path.join(REPO, "tools", "pack_digest.cpp"), os.path.join(CSRC, "pack.cpp"), "-o", exe],
                   check=True, timeout=300)
    got = subprocess.run([exe], check=True, timeout=60, capture_output=True, text=True).stdout.splitlines()
    with open(os.path.join(GOLDEN, "pack_digests.txt")) as f:
        want = [ln for ln in f.read().splitlines() if dev or " wino_x3 " not in ln]
    assert len(want) >= 33
    for g, w in zip(got, want):
        assert g == w
    assert len(got) == len(want)
