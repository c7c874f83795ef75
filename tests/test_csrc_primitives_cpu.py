"""The device primitives live in csrc/gad_dev.h and nowhere else (read from the sources as text, no GPU): a kernel file
does not call the LDS-DMA builtin, write a s_waitcnt itself, raise a raw barrier, restate Philox or wrap the 16x16x4 fp32 MFMA."""
import glob
import os
import re

import pytest

CSRC = os.path.join(os.path.dirname(__file__), "..", "group-attribution-for-diffusion-models_amd", "csrc")
HOME = "gad_dev.h"


def _sources():
    paths = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))
    assert len(paths) >= 20 and any(os.path.basename(p) == HOME for p in paths)
    return {os.path.basename(p): open(p).read() for p in paths}


ONLY_IN_HOME = {
    "the LDS-DMA builtin": r"__builtin_amdgcn_global_load_lds",
    "the s_waitcnt builtin": r"__builtin_amdgcn_s_waitcnt",
    "s_waitcnt inside an asm": r"\basm\b[^;]*s_waitcnt",
    "the raw barrier builtin": r"__builtin_amdgcn_s_barrier",
    "the Philox multiplier": r"0xD2511F53",
    "the 16x16x4 fp32 MFMA builtin": r"__builtin_amdgcn_mfma_f32_16x16x4f32",
}


@pytest.mark.parametrize("what", sorted(ONLY_IN_HOME))
def test_written_in_gad_dev_h_and_nowhere_else(what):
    pat = re.compile(ONLY_IN_HOME[what])
    where = sorted(name for name, text in _sources().items() if pat.search(text))
    assert where == [HOME], f"{what} occurs in {where}"


@pytest.mark.parametrize("name", ["xcd_remap", "philox4x32_10", "barrier_vm", "wait_vm"])
def test_defined_once_in_the_tree(name):
    pat = re.compile(r"__device__[^;{()]*\b%s\s*\([^;{]*\)\s*\{" % name)
    found = [(f, m.group(0)) for f, text in _sources().items() for m in pat.finditer(text)]
    assert [f for f, _ in found] == [HOME], found
