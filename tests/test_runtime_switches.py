"""The run-time switch table of INTEGRATION.md (section 3b) lists exactly the EAO_* environment variables the library reads."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def library_switches():
    names = set()
    for top in ("eao_fusion_amd/csrc", "include"):
        for d, _, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                if f.endswith((".hip", ".h", ".inc", ".cpp")):
                    names |= set(re.findall(r'getenv\("(EAO_[A-Z0-9_]+)"', open(os.path.join(d, f)).read()))
    return names


def table_switches():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    section = re.search(r"^## 3b\..*?$(.*?)^## ", text, re.M | re.S)
    assert section, "INTEGRATION.md has no section 3b"
    names = set()
    for line in section.group(1).splitlines():
        cells = line.split("|")
        if line.startswith("|") and len(cells) > 2:
            names |= set(re.findall(r"`(EAO_[A-Z0-9_]+)", cells[1]))
    return names


def test_switch_table_matches_library():
    lib, table = library_switches(), table_switches()
    assert lib, "no getenv(\"EAO_...\") found in the library sources"
    assert lib - table == set(), "read by the library, missing from INTEGRATION.md section 3b"
    assert table - lib == set(), "listed in INTEGRATION.md section 3b, not read by the library"
