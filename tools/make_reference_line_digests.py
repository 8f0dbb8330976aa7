"""Writes tests/golden/reference_chicdiff_R_digests.json: one-way digests of the reference's Chicdiff/R/chicdiff.R — a
truncated SHA-256 of every line in file order, and the set of digests of its normalised code lines — so that
tests/test_r_shim.py can check, without the reference tree, that r/patches/chicdiff_hip.patch applies to it and that the
R host in r/R/ shares few code lines with it.  The fixture holds no line of the reference, only digests.
usage: python tools/make_reference_line_digests.py <path to Chicdiff/R/chicdiff.R>"""
import hashlib
import importlib.util
import json
import os
import sys

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
OUT = os.path.join(ROOT, "tests", "golden", "reference_chicdiff_R_digests.json")

# the normalisation and the digest are the test's own (one definition)
spec = importlib.util.spec_from_file_location("test_r_shim", os.path.join(ROOT, "tests", "test_r_shim.py"))
t = importlib.util.module_from_spec(spec)
spec.loader.exec_module(t)

if len(sys.argv) != 2:
    raise SystemExit(__doc__)
raw = open(sys.argv[1], "rb").read()
lines = raw.decode("utf-8", errors="replace").split("\n")
if lines and lines[-1] == "":
    lines.pop()
fixture = {"source": "Chicdiff/R/chicdiff.R", "sha256": hashlib.sha256(raw).hexdigest(),
           "lines": [t._digest(l) for l in lines],
           "code_lines": sorted({t._digest(l) for l in t._code_lines(lines)})}
json.dump(fixture, open(OUT, "w"), indent=0)
print(len(fixture["lines"]), "lines,", len(fixture["code_lines"]), "distinct code lines ->", os.path.relpath(OUT, ROOT))
