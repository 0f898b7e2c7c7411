"""tools/plane_segmentation_walk.cpp built as a program of its own for the tests: csrc/plane_seg_internal.h under g++, nothing of it loaded into Python."""
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "plane_segmentation_walk.cpp")
_built = {}


def build(sanitize):
    """path of the program; sanitize: -fsanitize=address,undefined (the CPU tests), else -O2.  -ffp-contract=off either way, as the library."""
    if sanitize not in _built:
        d = tempfile.mkdtemp(prefix="eao_walk_")
        exe = os.path.join(d, "walk")
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
        subprocess.check_call([shutil.which("g++") or "g++", "-std=c++17", "-ffp-contract=off", "-Wall"] + flags + ["-o", exe, SRC])
        _built[sanitize] = exe
    return _built[sanitize]


def run(exe, mode, payload, *more):
    """the program's standard output on a file that holds payload"""
    with tempfile.NamedTemporaryFile(suffix=".in", delete=False) as f:
        f.write(payload if isinstance(payload, bytes) else payload.encode())
        path = f.name
    try:
        p = subprocess.run([exe, mode, path] + [str(m) for m in more], capture_output=True, text=True, timeout=120)
    finally:
        os.unlink(path)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-2000:]
    return p.stdout
