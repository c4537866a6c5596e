#!/usr/bin/env python3
"""Write tests/golden/reference_extract.json: what the reference-facing tests compare with, read from a reference tree.

The reference (PAM) is not part of this repository and is not needed to run the tests.  Where a checkout of it is at hand,
this script re-reads it with the `extract` functions of the two test modules and stores the result as data -- member names of
the coupler and DataManager headers, SHA-256 digests of the Dycore signature lines, the numeric literals of the generated
matrices, WENO weights and Kessler / sponge constants.  No source text of the reference is stored.

Usage:  python tests/golden/extract_reference.py REFERENCE_DIR [--check]
        --check: compare with the committed file instead of rewriting it (exit status 1 when they differ)
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "reference_extract.json")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import test_boundary_surface          # noqa: E402
import test_constants_vs_reference    # noqa: E402


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if len(args) != 1 or not os.path.isdir(args[0]):
        raise SystemExit(__doc__)
    ref = os.path.abspath(args[0])
    data = {"source": "read from the reference's headers by tests/golden/extract_reference.py",
            "boundary_surface": test_boundary_surface.extract(ref),
            "constants": test_constants_vs_reference.extract(ref)}
    text = json.dumps(data, indent=1, sort_keys=True) + "\n"
    if "--check" in sys.argv:
        same = os.path.exists(OUT) and open(OUT).read() == text
        print("reference_extract.json: %s" % ("up to date" if same else "DIFFERS"))
        sys.exit(0 if same else 1)
    with open(OUT, "w") as fh:
        fh.write(text)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
