"""Generates tests/golden/reference_api.json by asking the UNMODIFIED reference package (/root/reference/string_grouper,
v0.7.1) what tests/_reference_answers.py asks: its public and private surface, and ``_is_series_of_strings`` on every kind
of Series.  tests/test_host_api.py compares the mirror with the recorded answers.

Run:  python tests/golden/make_golden_api.py      (needs /root/reference; not run on the GPU box)
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)                                     # for ``tests`` and ``oracle`` (used by the shims)
sys.path.insert(0, os.path.join(ROOT, "tests", "ref_shims"))
sys.path.insert(0, "/root/reference")                        # must win over the repo's own drop-in alias

import string_grouper.string_grouper as ref  # noqa: E402

from tests import _reference_answers as A  # noqa: E402

assert ref.__file__.startswith("/root/reference"), "must import the reference package"

out = {"generator": "tests/golden/make_golden_api.py", "reference": "Bergvca/string_grouper v0.7.1",
       "surface": A.surface(ref), "series_validation": A.series_answers(ref.StringGrouper)}
with open(A.GOLDEN, "w") as f:
    json.dump(out, f, indent=1, sort_keys=True)
    f.write("\n")
print("wrote", A.GOLDEN)
