#!/usr/bin/env python3
"""Record the member-function signatures of the reference's ORBmatcher (include/ORBmatcher.h) and Optimizer (include/Optimizer.h) as DATA
-> tests/golden/ref_signatures.json, the fixture tests/test_standin_signatures.py compares the stand-ins of tests/cpp/integration/ref/ with.
Each signature is (name, parameter types in order, return type), normalised by that test's own parser (parameter names, defaults, `std::` and
white space dropped).

  python tools/gen_ref_signatures.py REFERENCE_DIR            # rewrite the fixture
  python tools/gen_ref_signatures.py REFERENCE_DIR --check    # exit 1 when the fixture differs from the reference's headers"""
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ref_signatures.json")
CLASSES = (("ORBmatcher", "include/ORBmatcher.h"), ("Optimizer", "include/Optimizer.h"))


def _parser():
    spec = importlib.util.spec_from_file_location("standin_signatures", os.path.join(ROOT, "tests", "test_standin_signatures.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.signatures


def parse(ref):
    signatures = _parser()
    out = {"source": "reference headers, parsed by tools/gen_ref_signatures.py: " + ", ".join("%s (class %s)" % (rel, cls) for cls, rel in CLASSES)}
    for cls, rel in CLASSES:
        sigs = signatures(open(os.path.join(ref, rel), encoding="utf-8", errors="replace").read(), cls)
        out[cls] = sorted([name, list(params), ret] for (name, params), ret in sigs.items())
    return out


def main(argv):
    if len(argv) < 2:
        sys.exit(__doc__)
    now = parse(argv[1])
    if "--check" in argv[2:]:
        same = json.load(open(FIXTURE)) == now
        print("fixture %s the reference's headers" % ("matches" if same else "DIFFERS FROM"))
        return 0 if same else 1
    with open(FIXTURE, "w") as f:
        json.dump(now, f, indent=1)
        f.write("\n")
    print("%s: %s" % (os.path.relpath(FIXTURE, ROOT), ", ".join("%s %d" % (cls, len(now[cls])) for cls, _ in CLASSES)))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
