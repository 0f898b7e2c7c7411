"""Every header of include/eaofusion/ compiles on its own: each includes what it uses, so a user may include any one of them first."""
import glob
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = sorted(glob.glob(os.path.join(ROOT, "include", "eaofusion", "*.h")))


def test_the_header_set_is_found():
    assert len(HEADERS) >= 21 and any(h.endswith("adapter_detail.h") for h in HEADERS)


@pytest.mark.parametrize("header", HEADERS, ids=[os.path.basename(h) for h in HEADERS])
def test_adapter_header_compiles_on_its_own(header):
    cc = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-DEAOFUSION_FORCE_CV_COMPAT", "-I", os.path.join(ROOT, "include"), "-x", "c++", header],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
