"""Generates tests/golden/reference_lines.json for tests/test_citations.py: the line count of every file of the
reference checkout that a `file:line` citation can name (no node_modules, no .git).  A list of names and numbers,
no file contents.  Run from the repo root with the checkout's path:

    python tests/golden/make_reference_index.py <reference checkout>
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

if __name__ == "__main__":
    from test_citations import reference_lines
    rec = reference_lines(sys.argv[1])
    with open(os.path.join(HERE, "reference_lines.json"), "w") as f:
        json.dump(dict(sorted(rec.items())), f, indent=0)
        f.write("\n")
    print(len(rec), "files")
