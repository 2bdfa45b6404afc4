#!/usr/bin/env python3
"""Record the usage surface of a `distance` binary as tests/cli_usage_outcomes.json.

    tools/record_cli_usage.py --cli /path/to/known-good/distance --commit <the commit it was built from>

The cases come from tests/cli_usage_cases.py; tests/test_cli_usage_table_host.py holds the tree's binary to the recorded
outcomes.  Record from a build of a commit whose messages are the ones to keep (before a change to parse_args: its
parent), never from the tree under test.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cli_usage_cases as cu  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cli", required=True, help="the binary to record")
    ap.add_argument("--commit", required=True, help="the commit that binary was built from")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "cli_usage_outcomes.json"))
    a = ap.parse_args()
    case_list = cu.cases()
    fixture = {"recorded_from": a.commit, "n_cases": len(case_list), "cases_sha256": cu.cases_digest(case_list)}
    fixture.update(cu.pack(cu.run_all(os.path.abspath(a.cli), case_list)))
    with open(a.out, "w") as fh:
        json.dump(fixture, fh, separators=(",", ":"))
        fh.write("\n")
    print(f"{len(case_list)} cases, {len(fixture['outcomes'])} distinct outcomes, {len(fixture['messages'])} messages, "
          f"{os.path.getsize(a.out)} bytes -> {a.out}")


if __name__ == "__main__":
    main()
