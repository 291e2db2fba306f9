"""The environment variables the library reads are the ones DESIGN.md lists
("Environment variables the library reads"): an experiment's switch is either
documented there or removed with the experiment."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read_in_code():
    names = set()
    for path in glob.glob(os.path.join(ROOT, "comdb2_amd", "csrc", "*")):
        if os.path.isfile(path) and path.endswith((".hip", ".cpp", ".h")):
            with open(path, encoding="utf-8") as f:
                names |= set(re.findall(r'getenv\(\s*"(HSC_[A-Z0-9_]+)"', f.read()))
    return names


def _listed_in_design():
    with open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8") as f:
        text = f.read()
    section = text.split("### Environment variables the library reads", 1)[1].split("\n## ", 1)[0]
    return set(re.findall(r"^\| `(HSC_[A-Z0-9_]+)` \|", section, re.M))


def test_env_knobs_match_design_table():
    code, doc = _read_in_code(), _listed_in_design()
    assert code and doc
    assert code == doc, f"read but not listed: {sorted(code - doc)}; listed but not read: {sorted(doc - code)}"
