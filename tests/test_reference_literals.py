"""Every fixture tests/golden/<feature>_constants.json is what its table in tools/reference_literals.py records, and -- where EAO_REFERENCE_DIR names a reference
tree -- what that tree's text says.  The feature tests hold our code to the fixtures; this file holds the fixtures to the reference."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import reference_literals as L  # noqa: E402

KEYS = {"name", "literal", "where"}
TYPED_KEYS = KEYS | {"type", "value", "note"}      # ref_constants.json (tests/test_ref_constants.py holds the three to tools/gen_ref_constants.py)


def _capture_group(rx, group):
    """the text of the regular expression's group-th capture group (the tables nest none)"""
    return re.findall(r"(?<!\\)\(((?:\\.|[^()\\])*)\)", rx)[group - 1]


@pytest.mark.parametrize("feature", sorted(L.TABLES))
def test_fixture_is_what_the_table_records(feature):
    fix, table = L.load(feature), L.TABLES[feature]
    assert [(r["name"], r["where"]) for r in fix] == [(name, "%s:%d" % (rel, line)) for name, rel, line, _rx, _group in table]
    assert all(set(r) == (TYPED_KEYS if feature == "ref" else KEYS) for r in fix)
    for r, (name, _rel, _line, rx, group) in zip(fix, table):
        assert re.compile(rx).groups >= group and re.fullmatch(_capture_group(rx, group), r["literal"]), (name, rx, group, r["literal"])
    assert L.two_spellings(fix) == []
    assert L.literals(feature) == {r["name"]: r["literal"] for r in fix}


@pytest.mark.parametrize("feature", sorted(L.TABLES))
def test_fixture_equals_the_reference_text(feature):
    ref = os.environ.get("EAO_REFERENCE_DIR")
    if not ref or not os.path.isdir(ref):
        pytest.skip("EAO_REFERENCE_DIR does not name a reference tree")
    assert L.parse(ref, feature) == [{k: r[k] for k in sorted(KEYS)} for r in L.load(feature)]
