"""Generates tests/golden/translated_subop.json: for every tests/golden/subop_*.json dump, the status, the plan text and the
placement report that `api.translate_subop_dump` gives, under the plan name tests/test_subop_dump.py uses for that dump
("subop_tpch_q6.json" → "tpch_q6", "subop_pat_mark.json" → "pat_mark", "subop_nl_band.json" → "nl_band").  The fixture pins
the translator's TEXT (tests/test_subop_dump.py compares it byte for byte), so it is recorded from the library of the commit
BEFORE a change that is meant to leave the translation alone, and regenerated only by a change that means to alter it.
(The fixture's own name does not begin with "subop_": every golden file that does is read as a dump by the tests.)

Run from the repo root where libldb_host.so has been built:  python tests/golden/make_subop_translated.py"""
import glob
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "lingo-db_amd"))

from lingodb_amd import api, capi  # noqa: E402

OUT = "translated_subop.json"


def translate(path):
    stem = os.path.splitext(os.path.basename(path))[0]
    with open(path) as f:
        text = f.read()
    try:
        plan, report = api.translate_subop_dump(text, stem[len("subop_"):])
        status = capi.LDB_OK
    except capi.LdbError as e:
        plan, report, status = "", e.report, e.status
    return stem, {"status": status, "plan": plan, "report": capi.host_lib().ldb_subop_report().decode()}


def main():
    paths = sorted(glob.glob(os.path.join(HERE, "subop_*.json")))
    doc = dict(translate(p) for p in paths)
    path = os.path.join(HERE, OUT)
    with open(path, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%s: %d dumps, %d with LDB_OK, %d bytes" % (OUT, len(doc), sum(v["status"] == capi.LDB_OK for v in doc.values()), os.path.getsize(path)))


if __name__ == "__main__":
    sys.exit(main())
