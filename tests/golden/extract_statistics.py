#!/usr/bin/env python3
"""Write tests/golden/statistics_extract.json: SHA-256 digests of the reference's signature lines of
modules::horizontal_average, modules::time_average_init and modules::time_average_accumulate, which
tests/test_statistics_modules.py compares with the adaptors under pam_amd/csrc/host/modules/.

The reference (PAM) is not part of this repository and is not needed to run the tests.  Where a checkout of it is at hand, this
script re-reads it; each digest is taken as tests/test_boundary_surface.py takes the Dycore's (the line and the next two joined,
whitespace and `pam::` removed, up to the opening brace).  No source text of the reference is stored.

Usage:  python tests/golden/extract_statistics.py REFERENCE_DIR [--check]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "statistics_extract.json")
sys.path.insert(0, os.path.dirname(HERE))

import test_boundary_surface as tb    # noqa: E402

# reference file -> the line numbers of the signatures recorded
LINES = {"pam_core/modules/horizontal_average.h": [25], "pam_core/modules/time_average.h": [8, 39]}


def extract(ref):
    out = {}
    for rel, lns in LINES.items():
        lines = open(os.path.join(ref, rel)).read().split("\n")
        for ln in lns:
            got = tb._norm(" ".join(lines[ln - 1:ln + 2]))
            out["%s:%d" % (rel, ln)] = tb._digest(got[:got.index("{")])
    return {"source": "read from the reference's module headers by tests/golden/extract_statistics.py", "signature_sha256": out}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if len(args) != 1 or not os.path.isdir(args[0]):
        raise SystemExit(__doc__)
    text = json.dumps(extract(os.path.abspath(args[0])), indent=1, sort_keys=True) + "\n"
    if "--check" in sys.argv:
        same = os.path.exists(OUT) and open(OUT).read() == text
        print("statistics_extract.json: %s" % ("up to date" if same else "DIFFERS"))
        sys.exit(0 if same else 1)
    with open(OUT, "w") as fh:
        fh.write(text)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
